// libecb -- equivalence-class builder for alntools' bam2ec / bam2emase hot path on MI355X (gfx950).
//
// What the reference does per alignment in Python (alntools/bam_utils.py:258-344), per merge (:680-724) and per EC
// (:788-847) is done here by these groups of kernels (DESIGN.md section 4 has the measurements behind the shapes):
//
//   k_stream   one pass over the record tuples (12 B/record, 16-byte loads).  Wave-autonomous: each wave owns a
//              contiguous slice of the stream and walks it in tiles of 512 records with wave-private LDS and no
//              workgroup barriers.  Per tile: (a) record filter (bam_utils.py:264-270) and read heads from the host's run
//              counter (:289-320); (b) one {locus -> haplotype mask} open-addressing table per read in LDS -- ds_cmpst on the
//              locus, ds_or of the haplotype bit: the duplicate collapse of :322-325 and the per-(EC, target, haplotype) bit
//              test of :800-819 in two LDS atomics.  A pass of that table spans as many tiles as fit; at its end (a "flush") each
//              table entry is hashed once and summed per read (a commutative set hash that only places the EC: identity is the
//              key itself, the stand-in for the sorted string key of :307) and (c) one lane per read looks its set up in the
//              global EC table -- hash, then an exact compare of the stored key -- or inserts it, and records the slot of the
//              read.  Founders' (locus, mask) pairs are copied from LDS into the slot / the key arena by the whole wave.
//              (csrc/k_stream.inc, compiled twice: passes of up to 64 reads at five waves per SIMD; passes of up to 128 reads with one-byte
//              masks at four, for batches of short reads -- chosen per batch when ecb_hint_reads has bounded the stream's reads.)
//   k_slow     the same for single reads that do not fit a tile or hit a full table (one workgroup per read).
//   k_count    reads per EC and first read per EC (:309-312, 688-698) from the per-read slots, without global atomics:
//              partition by slot range, count in LDS.
//   finalize   rank ECs by first appearance (bitmap + scan: :682-698), scan of row lengths, sort each row by locus and
//              emit CSR A / N (:835-847, bin_utils.py:208-211).
//   k_merge    multi-GPU: re-insert another rank's serialised table (the ordered merge of :680-724).
//   k_ms_*, k_msf*   multisample: (EC, cell, file) triples of the reads (one radix sort); cell order, minimum-count filter, EC re-rank
//              and CSC N in linear passes over them (bam_utils_multisample.py:503-636, 737-791).
//   k_cv_*     CSR(bitmask) -> per-haplotype CSC as a transposition of the non-zeros; k_cvu_* / k_cvb_*: back, as a union per column
//              in LDS hash tables and the same transposition (bin_utils.py:979-1028).
//
// Integer / indexing work only: no MFMA.  The bound is HBM bandwidth: the stream part of k_stream runs at the chip's streaming rate, what is
// left above it is the EC table's random lines sharing the memory system with the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ecb.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;

constexpr int TPB = 256;             // threads per workgroup (4 waves of 64)
constexpr u32 MAX_PROBE = 256;       // EC-table probes before a read is deferred to k_slow
constexpr u32 PENDING = 0xFFFFFFFFu;
constexpr u32 ARENA_CHUNK = 512;     // pairs a wave reserves from the key arena per global atomic
constexpr u32 QSTRIPES = 64;         // the deferred-read queue is filled in this many stripes, each with a counter of its own (queue_defer)
constexpr u32 ARENA_REGIONS = 64;    // the key arena has this many allocation cursors (see arena_alloc)
constexpr u32 MAX_LOCI = (1u << 26) - 2u;         // k_stream's LDS keys hold locus + 1 below the read's index within the pass: 26 bits (k_stream.inc) ...
constexpr u32 MAX_LOCI_SHORT = (1u << 25) - 2u;   // ... 25 in the kernel for short reads (seven bits of read index)
constexpr u32 INL = 5;               // (locus, mask) pairs of an EC's key held in its table slot; longer keys continue in the arena
constexpr u32 DEAD_KEY = 0xFFFFFFFFu;   // Slot::n1 of a slot whose key could not be stored (arena exhausted: the run fails)
constexpr u32 SPIN_MAX = 1u << 16;   // polls of a claimed slot's n1 before giving up (ERR_INTERNAL: the launch winds down; never seen)

constexpr u32 ERR_CONTRACT = 1u;     // device error bits (Counters::err)
constexpr u32 ERR_RANGE = 2u;
constexpr u32 ERR_ARENA = 4u;
constexpr u32 ERR_QUEUE = 8u;
constexpr u32 ERR_INTERNAL = 16u;
constexpr u32 ERR_COUNT = 32u;       // a count handed in by the caller does not fit the int32 of N

// One EC = one 64-byte line.  EC identity is EXACT: `lo` is only the hash that picks the slot; a lookup that finds its hash
// compares the read's {locus -> haplotype mask} set with the key stored in the slot, pair by pair, before it calls the slot
// its own (bam_utils.py:307-312 compares the sorted tid strings).  Two different target sets with the same 64-bit hash
// simply live in two slots.  Keys of up to INL loci sit in the line the lookup fetches anyway, so the compare costs no
// memory traffic; longer keys continue in the key arena.
// Life of a slot: lo 0 -> hash (atomicCAS: claimed); the claimant stores the pairs and the word {n1 = n + 1, off}, each
// with one 8-byte write-through store, in any order and without waiting for any of them.  A reader needs no ordering
// either: the haplotype mask of a key pair is never zero and slot and arena start out zeroed, so a key is complete exactly
// when n1 is set and its n masks are non-zero -- anything less is "not published yet" and is polled again.  Nothing ever
// changes lo, n1, off or a pair once written, until the table is cleared.
struct alignas(64) Slot {
    u64 lo;                          // 64-bit set hash, non-zero once claimed
    u32 n1;                          // 0 until the key is complete, then number of pairs + 1
    u32 off;                         // key pairs INL.. : arena[off .. off + n - INL)
    u32 count;                       // reads in this EC                       (k_count)
    u32 first_inv;                   // ~(smallest read index)                 (k_count; atomicMax on zero-initialised memory)
    uint2 pair[INL];                 // key pairs 0 .. min(n, INL): (locus, haplotype mask), in no particular order
};
static_assert(sizeof(Slot) == 64, "one EC per 64-byte line");
static_assert(offsetof(Slot, n1) == 8 && offsetof(Slot, off) == 12 && offsetof(Slot, count) == 16 && offsetof(Slot, first_inv) == 20,
              "k_count_bins reads {n1, off} and {count, first_inv} as 8-byte words");
// what ranks exchange (ecb_table_export_* / merge / adopt): 32 bytes per EC, its key pairs packed in a list of their own
struct Entry {
    u64 lo, reserved;
    u32 count, first_inv;
    u32 off, n;                      // key = pairs[off .. off + n), sorted by locus
};
static_assert(sizeof(Entry) == 32, "exchange format");

struct Counters {
    u64 all, valid;                  // records offered / passing the filter
    u64 arena_top;                   // pairs placed by ecb_table_adopt_device (dense from 0; an adopting handle allocates nothing else)
    u64 n_queue;                     // reads deferred to k_slow (k_sum_counts: the sum over the stripes below)
    u64 n_queue_s[QSTRIPES];         // ... counted per stripe of the queue (queue_defer)
    u64 n_ecs;                       // ECs created by k_slow / k_merge (k_stream's are counted by k_collect_new)
    u32 err;
    u32 full;                        // set when a read found no EC-table slot: workgroups park, host grows the table
    u64 arena_reg[ARENA_REGIONS];    // next free pair of every arena region
    u64 next_slice;                  // k_stream: next unclaimed slice of the batch (zeroed per launch)
    u64 n_mismatch;                  // exactness pass (ecb_verify_device): reads whose set differs from their EC's key
    u32 last_rid, pad_;              // read_id of the last record of the batch k_sum_counts closed (ecb_hint_reads: the host learns it here)
    u64 n_probe_tiles;               // tile visits on k_stream's probe-on path (records that found their first LDS slot taken), over the batches so far
};

// The key arena is cut into equal regions with a cursor each; a wave allocates from the region its index picks and moves
// on when that one is full.  One cursor for the whole arena is one address for every reservation of every wave:
// same-address atomics complete ~18 ns apart, and the 66 k chunk reservations of a C3 pass added 1.4 ms to k_stream.
// (Regions of at least 64 k pairs; small arenas have fewer.)  Keys are found through Slot::off, nothing needs the arena dense.
__host__ __device__ __forceinline__ u32 arena_regions(u64 arena_cap) { return (u32)(arena_cap >> 16 >= ARENA_REGIONS ? ARENA_REGIONS : (arena_cap >> 16 ? arena_cap >> 16 : 1)); }
__device__ __forceinline__ u64 arena_alloc(Counters* ctr, u64 arena_cap, u32 n, u32 hint) {
    const u32 R = arena_regions(arena_cap);
    const u64 per = arena_cap / R;
    for (u32 t = 0; t < R; ++t) {
        const u32 r = (hint + t) % R;
        const u64 at = atomicAdd(&ctr->arena_reg[r], (u64)n);     // (a failed try leaves the cursor past the end: that region is full)
        if (at + n <= (u64)(r + 1) * per) return at;
    }
    return ~0ull;
}

// ---------------------------------------------------------------------------------------------
// hashing: an EC is the SET of (locus, haplotype) targets of a read (bam_utils.py:307 builds a sorted string for the
// same purpose).  The set is held as {locus -> haplotype mask}; its hash is the sum over loci of a 64-bit mix of
// (locus, mask).  The sum commutes, so records need no sorting, and OR-ing haplotype bits makes duplicate
// (read, target) records vanish by itself.  The hash only places the EC in the table: equality is decided on the key.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 fmix32(u32 h) {           // murmur3 finaliser: a bijection with full avalanche
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ u64 pair_hash64(u32 locus, u32 mask) {
    // two finalisers instead of four: the hash only places an EC in the table (identity is the key), and what the sum over a
    // read's pairs needs is that the low word spreads over the slots and the high word differs where the low one collides
    const u32 h0 = fmix32(locus * 0x9E3779B1u + mask * 0x85EBCA77u + 0x7F4A7C15u);
    const u32 h1 = fmix32((h0 ^ locus) * 0xC2B2AE3Du + mask);
    return ((u64)h1 << 32) | h0;
}
// the sums of fmix32 outputs are already uniformly spread: the table hash is the sum itself (made non-zero)
__device__ __forceinline__ u64 finish_hash(u64 s0, u32 n) { return (s0 + ((u64)n << 32) + n) | 1ull; }

// record filter, bam_utils.py:264-270 (host bits 12/13 carry the two non-flag terms)
__device__ __forceinline__ bool rec_valid(u32 hf) {
    if (hf & 0x4u) return false;
    if (hf & 0x1u) {
        if ((hf & 0x80u) || !(hf & 0x2u) || (hf & (ECB_FLAG_MATE_OTHER_REF | ECB_FLAG_NEXT_POS_NEG))) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// EC-table lookup / insert with exact keys.
//   table_lookup: probes from j.  Plain loads: a cached line can only be an OLDER state of the slot (empty -> claimed ->
//     published, never back), so what a stale line can cost is an atomic or a trip through table_settle, never a wrong
//     answer: "empty" is re-checked by the CAS, "not published" and "hash equal, key different" are both settled on fresh
//     reads, and a match is a match (the pairs of a slot only ever go from zero to their final value).
//   table_settle: the slot carries our hash but its key was not (visibly) complete, or did not compare equal.  Polls n1
//     and re-reads the key with read-modify-write atomics, which execute at the memory side, and decides for good.
//   Callers that create a slot publish it (store off + pairs write-through, s_waitcnt vmcnt(0), then n1) BEFORE any lane
//   of their wave calls table_settle: the creator a lane waits for may sit in its own wave.
// Read counts and first appearances are NOT maintained here: per-read atomics on a skewed EC distribution run at
// ~5 G/s chip-wide (measured), so k_stream only records the slot of every read and k_count reduces them afterwards.
// ---------------------------------------------------------------------------------------------
enum { ST_NONE = 0, ST_LOOK, ST_HIT, ST_CREATED, ST_PENDING, ST_FULL, ST_OTHER, ST_STUCK, ST_CLAIM };   // (ST_CLAIM: k_stream's flush -- found empty, the claim not yet made)
enum { CMP_EQUAL = 0, CMP_DIFFERENT, CMP_INCOMPLETE, CMP_UNSURE };
struct SlotView { u32 n, off; uint2 p[INL]; };

__device__ __forceinline__ u64 fresh64(u64* p) { return atomicOr(p, 0ull); }      // a read that cannot be served from a stale cache line
__device__ __forceinline__ void store_wt64(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // write-through
__device__ __forceinline__ u64 pack2(uint2 v) { return ((u64)v.y << 32) | v.x; }
__device__ __forceinline__ uint2 unpack2(u64 v) { return make_uint2((u32)v, (u32)(v >> 32)); }
__device__ __forceinline__ void publish_key(Slot* s, u32 n1, u32 off) { store_wt64(reinterpret_cast<u64*>(&s->n1), ((u64)off << 32) | n1); }   // n1 and off: one word
// pair i of the key of a PUBLISHED slot, outside the kernels that publish (finalize, export, rehash): plain loads
__device__ __forceinline__ uint2 key_pair(const Slot& s, const uint2* arena, u32 i) { return i < INL ? s.pair[i] : arena[(u64)s.off + (i - INL)]; }
// ... and of a slot that may be in the middle of being published: a read that no cache can serve
__device__ __forceinline__ uint2 key_pair_fresh(Slot* s, uint2* arena, u32 off, u32 i) {
    return unpack2(fresh64(reinterpret_cast<u64*>(i < INL ? &s->pair[i] : arena + ((u64)off + (i - INL)))));
}

// ---------------------------------------------------------------------------------------------
// EC-table lookup / insert with exact keys.  A comparator has two forms:
//   quick(view)  on the line a lookup has just loaded: CMP_EQUAL (same size, every stored pair in my set), CMP_DIFFERENT (a
//                stored pair -- complete, since its mask is non-zero -- is not in my set, or the sizes differ), CMP_INCOMPLETE
//                (a mask still zero) or CMP_UNSURE (it would take more work to tell);
//   full(slot, n, off)   reads the key itself, fresh (read-modify-write atomics): the first three, after whatever work it takes.
//   table_lookup: probes from j, the whole line in one round trip.  Plain loads: a cached line can only be an OLDER state
//     of the slot (zeros where values will be), so what a stale line can cost is an atomic or a trip through table_settle,
//     never a wrong answer: "empty" is re-checked by the CAS, "not complete" is polled, and "equal" / "different" are
//     decided on pairs that are final.
//   table_settle: the slot carries our hash but its key was not (visibly) complete, or the quick look could not tell.
//     Polls with read-modify-write atomics, which execute at the memory side, until the key is whole, and decides.
//   Callers that create a slot publish it BEFORE any lane of their wave calls table_settle: the creator a lane waits for
//   may sit in its own wave.
//   (k_stream's flush does not call table_lookup: it reads lines and claims' answers the same way, but with the loads and the
//    claims of all its lanes in flight together -- k_stream.inc, phase (c).  k_slow, k_merge and the rehash do.)
// Read counts and first appearances are NOT maintained here: per-read atomics on a skewed EC distribution run at
// ~5 G/s chip-wide (measured), so k_stream only records the slot of every read and k_count reduces them afterwards.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ SlotView make_view(uint4 a, uint4 b, uint4 c, uint4 d) {
    SlotView v;
    v.n = a.z - 1u; v.off = a.w;
    v.p[0] = make_uint2(b.z, b.w); v.p[1] = make_uint2(c.x, c.y); v.p[2] = make_uint2(c.z, c.w);
    v.p[3] = make_uint2(d.x, d.y); v.p[4] = make_uint2(d.z, d.w);
    return v;
}
// The pairs of a key of at most RANKED_MAX pairs in ascending order of their loci: emit(rank, locus, mask) once per pair.  The key is held in
// registers and ranked with every index a compile-time constant: pairs picked by a run-time index (`key_pair(s, arena, j)` on a copy of the
// slot) put the copy in scratch memory and every step of the ranking behind a round trip to it -- k_emit_small 0.20 ms at C3 and 0.60 on the
// paralog stream.  A pair that is not there holds locus 2^32 - 1: it ranks behind everything and is not emitted.
constexpr u32 RANKED_MAX = 16;
template <class F>
__device__ __forceinline__ void ranked_pairs(const SlotView& v, const uint2* arena, F&& emit) {
    const u32 sn = v.n;
    u32 X[RANKED_MAX], Y[RANKED_MAX];
#pragma unroll
    for (u32 i = 0; i < INL; ++i) { X[i] = i < sn ? v.p[i].x : 0xFFFFFFFFu; Y[i] = v.p[i].y; }
    if (sn <= INL) {
#pragma unroll
        for (u32 i = 0; i < INL; ++i) {
            u32 r = 0;
#pragma unroll
            for (u32 j = 0; j < INL; ++j) r += X[j] < X[i] ? 1u : 0u;    // loci within a key are distinct
            if (i < sn) emit(r, X[i], Y[i]);
        }
    } else {                                         // ... the rest of a longer key from the arena, all loads in flight together
#pragma unroll
        for (u32 k = 0; k < RANKED_MAX - INL; ++k) {
            const uint2 t = INL + k < sn ? arena[(u64)v.off + k] : make_uint2(0xFFFFFFFFu, 0u);
            X[INL + k] = t.x; Y[INL + k] = t.y;
        }
#pragma unroll
        for (u32 i = 0; i < RANKED_MAX; ++i) {
            u32 r = 0;
#pragma unroll
            for (u32 j = 0; j < RANKED_MAX; ++j) r += X[j] < X[i] ? 1u : 0u;
            if (i < sn) emit(r, X[i], Y[i]);
        }
    }
}
// ... and of a longer key, by one wave: emit(rank, locus, mask) once per pair.  The loci are ranked out of LDS -- the wave's copy of them (`sx`: BIG_LDS
// words), read four at a time, every lane the same address -- where a rank used to be a walk over the key in global memory per pair: 700 x 700
// loads for a read of 700 loci (k_emit_big 6 ms for the 39 k long ECs of tools/slow_path.py; profiles/r04_long_reads.txt).  Keys of more than
// BIG_LDS pairs walk the key in memory as before.
constexpr u32 BIG_LDS = 2048;                   // 8 KB per wave
template <class F>
__device__ __forceinline__ void ranked_pairs_wave(const Slot& s, const uint2* arena, u32 sn, u32* sx, u32 lane, F&& emit) {
    const bool in_lds = sn <= BIG_LDS;
    if (in_lds) {
        for (u32 i = lane; i < sn; i += 64) sx[i] = key_pair(s, arena, i).x;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    for (u32 i = lane; i < sn; i += 64) {
        const uint2 pi = key_pair(s, arena, i);
        u32 r = 0;
        if (in_lds) {
            u32 j = 0;
            for (; j + 4u <= sn; j += 4u) {
                const uint4 v = *reinterpret_cast<const uint4*>(&sx[j]);
                r += (v.x < pi.x ? 1u : 0u) + (v.y < pi.x ? 1u : 0u) + (v.z < pi.x ? 1u : 0u) + (v.w < pi.x ? 1u : 0u);
            }
            for (; j < sn; ++j) r += sx[j] < pi.x ? 1u : 0u;
        } else {
            for (u32 j = 0; j < sn; ++j) r += key_pair(s, arena, j).x < pi.x;        // loci within a key are distinct
        }
        emit(r, pi.x, pi.y);
    }
    if (in_lds) {                                  // (the wave's next key overwrites the copy)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
// -DECB_TIMING: what the waves of a launch did to each other OUTSIDE k_stream's flush (which counts its own, k_stream.inc) -- in k_slow and
// k_merge, the callers of table_lookup: claims lost to another hash [0] and to a founder with the same hash [1], lookups settled on a slot
// that carries their hash (table_settle in k_merge; same_key in k_slow, which compares every such slot) [2], and those of them that ended on
// the other key of the hash [3].  One device-wide word each, read and zeroed by ecb_timing_race (tools/racing_founders.py).
#ifdef ECB_TIMING
__device__ u64 g_race[4];
#define RACE(i) atomicAdd(&g_race[i], 1ull)
#else
#define RACE(i) do { } while (0)
#endif
template <class Cmp>
__device__ __forceinline__ int table_lookup(Slot* table, u64 cap_mask, u64 lo, u64& j, u32& probes, const Cmp& cmp, u32 abl = 0u, u32* first_inv_seen = nullptr) {
    for (; probes < MAX_PROBE; ++probes, j = (j + 1) & cap_mask) {
        Slot* s = table + j;
        const uint4* q = reinterpret_cast<const uint4*>(s);
        if (first_inv_seen) *first_inv_seen = 0u;
        uint4 a = q[0], b = a, c = a, d = a;                      // lo, n1, off | count, first_inv, pair 0 | pairs 1, 2 | pairs 3, 4
        if (!(abl & 16u)) { b = q[1]; c = q[2]; d = q[3]; }       // (profiling only: 16 = first 16 bytes only, 8 = no key compare)
        u64 clo = ((u64)a.y << 32) | a.x;
        if (clo == 0ull) {
            clo = atomicCAS(&s->lo, 0ull, lo);
            if (clo == 0ull) return ST_CREATED;
            if (clo == lo) { RACE(1); return ST_PENDING; }        // claimed with our hash a moment ago: its key decides
            RACE(0);
            continue;
        }
        if (clo != lo) continue;
        if (a.z == 0u) return ST_PENDING;
        if (a.z == DEAD_KEY) continue;
        if (first_inv_seen) *first_inv_seen = b.y;                 // (what this line -- possibly an old copy -- shows of the EC's first read)
        if (abl & 8u) return ST_HIT;
        const int r = cmp.quick(make_view(a, b, c, d));
        if (r == CMP_EQUAL) return ST_HIT;
        if (r != CMP_DIFFERENT) return ST_PENDING;
    }                                                             // (same hash, another key: a true collision takes the next slot)
    return ST_FULL;
}
template <class Cmp>
__device__ __forceinline__ int table_settle(Slot* s, const Cmp& cmp) {
    for (u32 spin = 0; spin < SPIN_MAX; ++spin) {
        const u64 w = fresh64(reinterpret_cast<u64*>(&s->n1));
        const u32 n1 = (u32)w;
        if (n1 == DEAD_KEY) return ST_OTHER;
        if (n1) {
            const int r = cmp.full(s, n1 - 1u, (u32)(w >> 32));
            if (r == CMP_EQUAL) return ST_HIT;
            if (r == CMP_DIFFERENT) return ST_OTHER;
        }
        __builtin_amdgcn_s_sleep(4);
    }
    return ST_STUCK;
}

// ---------------------------------------------------------------------------------------------
// k_stream -- wave-autonomous: every wave owns a contiguous slice of the record stream and walks it in
// tiles of WT records with wave-private LDS and no workgroup barriers, so the 16 waves of a CU overlap
// each other's HBM and EC-table latency.  Per tile and lane: 8 records (2 x 16-byte loads per stream).
// ---------------------------------------------------------------------------------------------
#ifndef ECB_RPL
#define ECB_RPL 8
#endif
constexpr int RPL = ECB_RPL;         // records per lane per tile: groups of 4 consecutive records (one 16-byte load per stream)
static_assert(RPL == 8, "only 8 records per lane is validated (16 was measured: 233 VGPRs, 2 waves/SIMD, 11-25 % slower; it also needs a 32-bit ent[])");
constexpr int NG = RPL / 4;          // groups; group g of lane l holds records 256 g + 4 l .. + 3 of the tile
constexpr int WT = 64 * RPL;         // records per wave tile
constexpr int NWAVE = TPB / 64;
// What k_stream needs once in a while sits behind ONE pointer (scalar registers are what this kernel runs out of: every
// kernel argument occupies a pair for the whole launch, and what does not fit is shuffled through vector lanes).
struct StreamCold {
    uint2* arena; u64 arena_cap;
    u64* queue; u64 queue_cap;       // head record index of deferred reads
    u64* resume;                     // per slice {where a relaunch takes it up, records counted up to}
    u32* wave_counts;                // per wave {records offered, records valid, ECs created}: summed by k_sum_counts
    u64* wave_arena;                 // per wave {start, pairs left} of its arena reservation, kept from launch to launch
    u64* timing;                     // profiling only (-DECB_TIMING): clocks per phase, summed over waves
    u64 chunk;                       // records per slice (a multiple of WT)
    u32 prev_rid;                    // read_id of the record before this batch (0xFFFFFFFF at stream start)
    // ECB_F_RANGES (k_stream<false, true>): reference_start of every record and the per-(locus, haplotype) extremes
    const int* pos; int2* rng; u32 n_loci, n_haps;     // rng[locus * n_haps + hap] = {min, max}: one 8-byte load per record
};
// A read k_stream hands to k_slow (longer than a pass carries, or bounced off a full table): its head goes into one of QSTRIPES stretches of the
// queue, picked by a hash of the head, each with its own counter.  (One counter for all: a stream with 1 % of reads of 700 loci made 200 k
// atomics on one address -- ~75 ns apiece at the memory side, in order: 15 ms on a 1 ms kernel, sat out by whatever the waves waited for next.
// profiles/r04_long_reads.txt)  k_queue_compact closes the stretches up for k_slow.
__device__ __forceinline__ void queue_defer(Counters* ctr, const StreamCold* C, u64 head) {
    const u32 st = (u32)((head * 0x9E3779B97F4A7C15ull) >> 58);
    static_assert(QSTRIPES == 64, "six bits of the hash pick the stripe");
    const u64 seg = C->queue_cap / QSTRIPES;
    const u64 qi = atomicAdd(&ctr->n_queue_s[st], 1ull);
    if (qi < seg) C->queue[(u64)st * seg + qi] = head; else atomicOr(&ctr->err, ERR_QUEUE);
}
// Phases of k_stream can be switched off at run time in a profiling build (libecb_ablate.so: tools/pmc_ladder.sh, tools_ablate.sh);
// the product build has the tests compiled out -- they cost a scalar register and a handful of branches per tile.
#ifdef ECB_ABLATE_RT
#define ABL(A, bits) ((A).ablate & (bits))
#else
#define ABL(A, bits) 0u
#endif
struct StreamArgs {
    const u32* rid; const u32* loc; const u32* hf;
    u64 n;
    Slot* table; u64 cap_mask;
    Counters* ctr;
    u32* read_slot;                  // slot of every read (indexed by read_id)
    u64 reads_hi;                    // read_slot holds [0, reads_hi): a read index beyond it is a broken run counter
    const StreamCold* cold;
    u32 ablate;                      // profiling builds only (-DECB_ABLATE_RT, env ECB_ABLATE): 1 = stop after (a), 2 = after (b), 4 = no EC table, 8 / 16 / 32 see table_lookup
    // ECB_F_RANGES (k_stream<false, true>) reads these two HERE and not behind `cold`: a pointer loaded from memory has no address space the compiler
    // knows, and the position stream and the range table were FLAT loads and atomics (57 of them in that compilation); the other compilations never
    // touch the two words, which then cost them nothing
    const int* pos; int2* rng;
};
// Words from one tile of a stream to the next: 512 = three arrays (ecb_push_device); 1536 = whole tiles, a tile's 512 read ids, 512 loci and 512
// haplotype/flag words side by side (ecb_push_device_tiled: rid = base, loc = base + 512, hf = base + 1024).  Read off the pointers -- three arrays
// that sit like this hold at most one tile, for which the two readings are the same -- rather than passed: a kernel argument is a scalar register
// pair for the whole launch, and the stream kernel spills them.
__device__ __forceinline__ u32 stream_tw(const u32* rid, const u32* loc, const u32* hf) { return (loc == rid + 512 && hf == rid + 1024) ? 1536u : 512u; }
#define A_TW(A) stream_tw((A).rid, (A).loc, (A).hf)
// record i of a stream whose tiles are tw words apart
__host__ __device__ __forceinline__ u64 rec_at(u64 i, u32 tw) { return (i >> 9) * (u64)tw + (i & 511ull); }

__device__ __forceinline__ void wave_sync() {   // orders this wave's LDS traffic (lanes run in lockstep)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// Wave-wide sums and scans on the DPP cross-lane paths of the VALU (row_shr within rows of 16 lanes, then row_bcast:15 / :31
// across rows): six dependent VALU ops instead of six dependent trips through the LDS crossbar (ds_bpermute, which is
// what __shfl* compile to) -- the latter were ~700 clocks of latency per use.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u32 dpp_add(u32 v) { return v + (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ u32 wave_incl_scan(u32 v) {
    v = dpp_add<0x111, 0xf>(v); v = dpp_add<0x112, 0xf>(v); v = dpp_add<0x114, 0xf>(v); v = dpp_add<0x118, 0xf>(v);   // row_shr:1,2,4,8
    v = dpp_add<0x142, 0xa>(v);            // row_bcast:15 -> rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);            // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ u32 wave_sum(u32 v) { return (u32)__builtin_amdgcn_readlane((int)wave_incl_scan(v), 63); }
__device__ __forceinline__ u32 lane_above(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }   // wave_shr:1 (lane 0 gets 0)
__device__ __forceinline__ int clamp04(int x, int, int) { return min(max(x, 0), 4); }   // v_med3_i32

struct TileRegs { u32 rr[RPL], ll[RPL], hh[RPL]; };


// -DECB_TIMING: profiling build.  Every wave adds up the shader clocks it spends in each phase of a tile (stalls are
// charged to the phase whose s_waitcnt sits them out); k_stream adds them into StreamArgs::timing[8].
#ifdef ECB_TIMING
#define ECB_TIMING_WORDS 20          // 0 - 6 clocks per phase | 7 probe-on tiles | 8 - 14 table trips per lookup | 15 - 18 lost claims and settles | 19 spare
#define TICK(i) do { const u64 t_ = __builtin_readcyclecounter(); tacc[i] += t_ - tlast; tlast = t_; } while (0)
#else
#define TICK(i) do { } while (0)
#endif

// First record of read `rd` among records [b, e) -- the run counter never decreases, and it steps ON a read's first record
// (the rare paths that hand a read to k_slow ask; nothing on the way of an ordinary tile keeps head positions)
__device__ __forceinline__ u64 tile_head(const u32* rid, u64 b, u64 e, u32 rd, u32 tw) {
    while (b < e) { const u64 m = b + ((e - b) >> 1); if ((int)(rid[rec_at(m, tw)] - rd) < 0) b = m + 1; else e = m; }
    return b;
}
__device__ __forceinline__ void load_tile(const StreamArgs& A, u64 tb, u64 te, u32 lane, TileRegs& R) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    tb = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(tb >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)tb);   // (wave-uniform: say so)
    if (tb + (u64)WT <= te) {
        // a whole tile: wave-uniform base (scalar registers) + 16 bytes per lane, the second group 4 KB on -- the address costs
        // one shift per tile, not six 64-bit additions
        // (non-temporal: the stream is read once; without the hint it pushes the EC table's lines out of L2 -- measured 3 %)
        const u64 tbw = (tb >> 9) * (u64)A_TW(A);              // (tb is a tile boundary)
        const char* pr = reinterpret_cast<const char*>(A.rid + tbw);
        const char* pl = reinterpret_cast<const char*>(A.loc + tbw);
        const char* ph = reinterpret_cast<const char*>(A.hf + tbw);
        const u32 off = lane * 16u;                      // (32 bits: the loads take it as an offset to the scalar base)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pr + (off + (u32)g * 1024u)));
            R.rr[4 * g] = v.x; R.rr[4 * g + 1] = v.y; R.rr[4 * g + 2] = v.z; R.rr[4 * g + 3] = v.w;
            v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pl + (off + (u32)g * 1024u)));
            R.ll[4 * g] = v.x; R.ll[4 * g + 1] = v.y; R.ll[4 * g + 2] = v.z; R.ll[4 * g + 3] = v.w;
            v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ph + (off + (u32)g * 1024u)));
            R.hh[4 * g] = v.x; R.hh[4 * g + 1] = v.y; R.hh[4 * g + 2] = v.z; R.hh[4 * g + 3] = v.w;
        }
        return;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {                      // the stream's last tile: record by record
        const u64 i0 = tb + (u64)g * 256 + 4u * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < te;
            R.rr[4 * g + j] = A.rid[rec_at(in ? i0 + j : te - 1, A_TW(A))];          // (past the end: the last read id again -- no step, no head)
            R.ll[4 * g + j] = in ? A.loc[rec_at(i0 + j, A_TW(A))] : 0u;
            R.hh[4 * g + j] = in ? A.hf[rec_at(i0 + j, A_TW(A))] : 0x4u;
        }
    }
}

// ECB_F_RANGES: the fourth stream of a tile, same shape as load_tile's three
__device__ __forceinline__ void load_pos(const int* pos, u64 tb, u64 te, u32 lane, int* P) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    tb = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(tb >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)tb);
    if (tb + (u64)WT <= te) {
        const char* pp = reinterpret_cast<const char*>(pos + tb);
        const u32 off = lane * 16u;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const i32x4 v = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(pp + (off + (u32)g * 1024u)));
            P[4 * g] = v.x; P[4 * g + 1] = v.y; P[4 * g + 2] = v.z; P[4 * g + 3] = v.w;
        }
        return;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const u64 i0 = tb + (u64)g * 256 + 4u * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) P[4 * g + j] = i0 + j < te ? pos[i0 + j] : 0;
    }
}

// k_stream itself, twice (see k_stream.inc): the geometry of a pass is a compile-time matter (LDS per wave, waves per SIMD, key bits)
#define ECB_KS_SHORT 0
#define ECB_KS_PAR 0
namespace ks_std {
#include "k_stream.inc"
}
#undef ECB_KS_SHORT
#define ECB_KS_SHORT 1
namespace ks_short {
#include "k_stream.inc"
}
#undef ECB_KS_SHORT
#undef ECB_KS_PAR
#define ECB_KS_SHORT 0
#define ECB_KS_PAR 1
namespace ks_par {
#include "k_stream.inc"
}
#undef ECB_KS_PAR
#undef ECB_KS_SHORT

// resume points of a fresh batch: slice b starts (and has counted its records up to) record b * chunk
// (ctr: the per-launch words of the batch's first launch are zeroed here too -- three memsets fewer in front of k_stream)
__global__ void k_init_resume(u64* resume, u64 slices, u64 chunk, Counters* ctr = nullptr) {
    const u64 b = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (b < slices) { resume[2 * b] = b * chunk; resume[2 * b + 1] = b * chunk; }
    if (b == 0 && ctr) { ctr->n_queue = 0; ctr->full = 0; ctr->next_slice = 0; }
    if (b < QSTRIPES && ctr) ctr->n_queue_s[b] = 0;
}

__global__ __launch_bounds__(1024) void k_sum_counts(const u32* wave_counts, u64 waves, Counters* ctr, u32 verify, u64 offered, u64 queue_cap, const u32* d_last = nullptr) {
    __shared__ u64 s[3][16];
    u64 a = 0, v = 0, e = 0;
    for (u64 i = threadIdx.x; i < waves; i += 1024) { a += wave_counts[3 * i]; v += wave_counts[3 * i + 1]; e += wave_counts[3 * i + 2]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d); v += __shfl_xor(v, d); e += __shfl_xor(e, d); }
    if ((threadIdx.x & 63u) == 0) { s[0][threadIdx.x >> 6] = a; s[1][threadIdx.x >> 6] = v; s[2][threadIdx.x >> 6] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = v = e = 0;
        for (int k = 0; k < 16; ++k) { a += s[0][k]; v += s[1][k]; e += s[2][k]; }
        if (verify) ctr->n_mismatch += e;                  // the exactness pass counts differing reads, and recounts nothing
        else { ctr->all += offered; ctr->valid += v; ctr->n_ecs += e; ctr->n_probe_tiles += a; }
        if (d_last) ctr->last_rid = *d_last;
        u64 nq = 0;                                        // deferred reads: what the stripes of the queue hold (a stripe that ran over has said so: ERR_QUEUE)
        for (u32 st = 0; st < QSTRIPES; ++st) nq += min(ctr->n_queue_s[st], queue_cap / QSTRIPES);
        ctr->n_queue = nq;
    }
}
// the stripes of the deferred-read queue, closed up: one workgroup per stripe
__global__ void k_queue_compact(const u64* queue, u64 queue_cap, const Counters* ctr, u64* out) {
    const u64 seg = queue_cap / QSTRIPES;
    u64 at = 0;
    for (u32 st = 0; st < blockIdx.x; ++st) at += min(ctr->n_queue_s[st], seg);
    const u64 n = min(ctr->n_queue_s[blockIdx.x], seg);
    for (u64 i = threadIdx.x; i < n; i += blockDim.x) out[at + i] = queue[(u64)blockIdx.x * seg + i];
}

// ---------------------------------------------------------------------------------------------
// k_count: reads per EC and first appearance per EC (bam_utils.py:309-312, 688-698), reduced from the
// per-read slot ids without global atomics: partition the (slot, read) pairs by slot range (LDS
// histogram, scan, scatter), then one workgroup per range counts in LDS and owns its slots' counters.
// ---------------------------------------------------------------------------------------------
constexpr u32 BIN_BITS = 14;                   // slots per range = LDS bins of one k_count_bins workgroup: 2^14 (64 KB of LDS, two workgroups per CU;
                                               // 2^13 made the partition's runs half as long: +0.08 ms at C3) up to a table of 2^27 slots,
constexpr u32 MAX_BIN_BITS = 15;               // 2^15 (128 KB) beyond -- a run-time argument `bb`, chosen per stream (ensure_counts)
constexpr u32 MIN_BIN_BITS = 11;
constexpr u32 MAX_BUCKETS = 8192;
static_assert(MAX_BIN_BITS <= 16, "a slot's index within its range is kept in 16 bits (k_part_scatter*, k_count_bins)");              // LDS histogram of the partition passes  (=> at most 2^28 slots)

// Partition passes: few, fat workgroups.  Every workgroup keeps one open line per range in flight (2 048 of them at C3); with
// 512 workgroups of 1 024 threads those lines stay in L2 until they are full far more often than with 1 024 x 256
// (measured: -0.25 ms of 1.4 at C3; non-temporal stores, which skip that write-combining, cost +3.5 ms).
constexpr int TPB_PART = 1024;
constexpr u32 PART_G = 512;
// reads per workgroup of the partition passes (the same cut in all of them): a multiple of 4, so that a workgroup's first read sits on a 16-byte boundary
__device__ __forceinline__ u64 part_per(u64 n_reads, u64 G) { return (((n_reads + G - 1) / G) + 3ull) & ~3ull; }
__global__ __launch_bounds__(TPB_PART) void k_part_hist(const u32* read_slot, u64 n_reads, u32 n_buckets, u32 bb, u32* hist) {
    extern __shared__ u32 sh[];
    const u64 G = gridDim.x, g = blockIdx.x, per = part_per(n_reads, G);
    const u64 r0 = min(g * per, n_reads), r1 = min(r0 + per, n_reads);
    for (u32 b = threadIdx.x; b < n_buckets; b += TPB_PART) sh[b] = 0;
    __syncthreads();
    // 16 bytes per lane where the range allows (which element a thread counts does not matter); the ragged ends one by one
    const u64 a0 = min((r0 + 3) & ~3ull, r1), a1 = max(r1 & ~3ull, a0);
    for (u64 r = r0 + threadIdx.x; r < a0; r += TPB_PART) { const u32 s = read_slot[r]; if (s != PENDING) atomicAdd(&sh[s >> bb], 1u); }
    for (u64 r = a0 + 4ull * threadIdx.x; r < a1; r += 4ull * TPB_PART) {
        const uint4 v = *reinterpret_cast<const uint4*>(read_slot + r);
        if (v.x != PENDING) atomicAdd(&sh[v.x >> bb], 1u);
        if (v.y != PENDING) atomicAdd(&sh[v.y >> bb], 1u);
        if (v.z != PENDING) atomicAdd(&sh[v.z >> bb], 1u);
        if (v.w != PENDING) atomicAdd(&sh[v.w >> bb], 1u);
    }
    for (u64 r = a1 + threadIdx.x; r < r1; r += TPB_PART) { const u32 s = read_slot[r]; if (s != PENDING) atomicAdd(&sh[s >> bb], 1u); }
    __syncthreads();
    for (u32 b = threadIdx.x; b < n_buckets; b += TPB_PART) hist[(u64)b * G + g] = sh[b];
}

__global__ __launch_bounds__(TPB_PART) void k_part_scatter(const u32* read_slot, u64 n_reads, u32 n_buckets, u32 bb, const u32* offs,
                                                      u16* pairs) {
    extern __shared__ u32 sh[];
    const u64 G = gridDim.x, g = blockIdx.x, per = part_per(n_reads, G);
    const u64 r0 = min(g * per, n_reads), r1 = min(r0 + per, n_reads);
    for (u32 b = threadIdx.x; b < n_buckets; b += TPB_PART) sh[b] = offs[(u64)b * G + g];
    __syncthreads();
    // four reads per thread and trip: their LDS cursor bumps are independent, so the round trips overlap
    for (u64 rb = r0; rb < r1; rb += 4 * TPB_PART) {
        u32 s[4], pos[4];
        u64 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = rb + (u64)k * TPB_PART + threadIdx.x;
            s[k] = r[k] < r1 ? read_slot[r[k]] : PENDING;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (s[k] != PENDING) pos[k] = atomicAdd(&sh[s[k] >> bb], 1u);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (s[k] != PENDING) pairs[pos[k]] = (u16)(s[k] & ((1u << bb) - 1u));
    }
}

// (Elements are slot ids alone: the first read of an EC is kept current by k_stream itself -- the lookup has the slot's line in
//  hand and adds an atomicMax only when its read is earlier than what the line shows -- so nothing but counts is left here.
//  And within its range a slot id is its low `bb` <= 15 bits: the partitioned elements are 2 bytes each, half the bytes to
//  write here and to read in k_count_bins.)
// The scatter with its elements sorted by range in LDS first: a workgroup takes STAGE reads at a time, ranks them within their
// range (LDS counters), lays them out range by range in LDS and writes them from there -- elements of one range leave in
// runs of consecutive addresses (STAGE / n_buckets of them on average) instead of one 8-byte store per lane and range.
constexpr u32 STAGE = 8 * TPB_PART;            // 8 192 elements = 32 KB of LDS
constexpr u32 STAGE_MAX_BUCKETS = 4096;        // 3 x 16 KB of counters / starts / cursors beside the stage
__global__ __launch_bounds__(TPB_PART) void k_part_scatter_staged(const u32* read_slot, u64 n_reads, u32 n_buckets, u32 bb, const u32* offs,
                                                             u16* pairs) {
    extern __shared__ u32 sh[];                   // cnt[nb] | start[nb] | gcur[nb] | stage[STAGE]
    u32 *cnt = sh, *start = sh + n_buckets, *gcur = sh + 2 * n_buckets;
    u32* stage = sh + 3 * n_buckets;
    __shared__ u32 s_wave[TPB_PART / 64];
    const u64 G = gridDim.x, g = blockIdx.x, per = part_per(n_reads, G);
    const u64 r0 = min(g * per, n_reads), r1 = min(r0 + per, n_reads);
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u32 bpt = (n_buckets + TPB_PART - 1) / TPB_PART;            // ranges per thread in the scan (1 .. 4)
    for (u32 b = tid; b < n_buckets; b += TPB_PART) gcur[b] = offs[(u64)b * G + g];
    for (u64 rb = r0; rb < r1; rb += STAGE) {
        for (u32 b = tid; b < n_buckets; b += TPB_PART) cnt[b] = 0;
        __syncthreads();
        u32 s[8], lr[8];
#pragma unroll
        for (int k4 = 0; k4 < 2; ++k4) {                  // 16 bytes per lane and load (which element a thread takes does not matter)
            const u64 r = rb + ((u64)k4 * TPB_PART + tid) * 4u;
            if (r + 4 <= r1) {
                const uint4 v = *reinterpret_cast<const uint4*>(read_slot + r);
                s[4 * k4] = v.x; s[4 * k4 + 1] = v.y; s[4 * k4 + 2] = v.z; s[4 * k4 + 3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) s[4 * k4 + j] = r + j < r1 ? read_slot[r + j] : PENDING;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (s[k] != PENDING) lr[k] = atomicAdd(&cnt[s[k] >> bb], 1u);
        __syncthreads();
        // exclusive scan of cnt[] -> start[]: bpt consecutive ranges per thread, DPP scan per wave, wave totals through LDS
        u32 mine = 0;
        for (u32 j = 0; j < bpt; ++j) { const u32 b = tid * bpt + j; mine += b < n_buckets ? cnt[b] : 0u; }
        const u32 incl = wave_incl_scan(mine);
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        u32 run = incl - mine;
        for (u32 k = 0; k < w; ++k) run += s_wave[k];
        for (u32 j = 0; j < bpt; ++j) { const u32 b = tid * bpt + j; if (b < n_buckets) { start[b] = run; run += cnt[b]; } }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (s[k] != PENDING) stage[start[s[k] >> bb] + lr[k]] = s[k];
        __syncthreads();
        u32 n_here = 0;
        for (u32 k = 0; k < TPB_PART / 64; ++k) n_here += s_wave[k];
        for (u32 i = tid; i < n_here; i += TPB_PART) {
            const u32 e = stage[i];
            const u32 b = e >> bb;
            pairs[gcur[b] + (i - start[b])] = (u16)(e & ((1u << bb) - 1u));
        }
        __syncthreads();
        for (u32 b = tid; b < n_buckets; b += TPB_PART) gcur[b] += cnt[b];
    }
}

constexpr int TPB_COUNT = 1024;
// A hot EC makes its range the tail of the kernel (C2: one range of 512 held 4 % of the reads): the host cuts ranges
// far above the average into pieces.  One piece = one workgroup; the pieces of a cut range add into the slots with
// atomics, whole ranges are the only writer of their slots and just store.
struct CountWork { u32 bucket, start, end, shared; };
// The work list is built on the device (one workgroup: a few thousand ranges), so that nothing between the stream kernel and
// the CSR waits for the host.  work[0 .. *n_work): whole ranges, or pieces of `piece` elements of a range far above the average.
__global__ __launch_bounds__(1024) void k_build_work(const u32* offs, u32 G, const u64* total, u32 n_buckets, u32 piece, CountWork* work, u32 max_work, u32* n_work) {
    __shared__ u32 s_w[16];
    __shared__ u32 s_carry;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u32 b0 = 0; b0 < n_buckets; b0 += 1024) {
        const u32 b = b0 + tid;
        u32 s0 = 0, s1 = 0, np = 0;
        if (b < n_buckets) { s0 = offs[(u64)b * G]; s1 = b + 1 < n_buckets ? offs[(u64)(b + 1) * G] : (u32)*total; }      // (a range starts where its first workgroup's elements do)
        const u32 len = s1 - s0;
        const bool cut = len > piece + piece / 2;
        if (len) np = cut ? (len + piece - 1) / piece : 1u;
        const u32 incl = wave_incl_scan(np);
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        u32 at = s_carry + incl - np, tot = 0;
        for (u32 k = 0; k < 16; ++k) { if (k < w) at += s_w[k]; tot += s_w[k]; }
        for (u32 k = 0; k < np; ++k)
            if (at + k < max_work) work[at + k] = cut ? CountWork{b, s0 + k * piece, min(s0 + (k + 1) * piece, s1), 1u} : CountWork{b, s0, s1, 0u};
        __syncthreads();
        if (tid == 0) s_carry += tot;
        __syncthreads();
    }
    if (tid == 0) *n_work = min(s_carry, max_work);
}
// sink (optional): what finalize's k_compact would otherwise find by scanning the whole table -- see the end of the kernel
struct CompactSink { u32* list; u64 max_list; u64* n_list; u32* bitmap; u64 n_bits; uint2* list_fn; };
__global__ __launch_bounds__(TPB_COUNT) void k_count_bins(const u16* pairs, const CountWork* work, const u32* n_work, u32 bb, Slot* table, CompactSink sink) {
    extern __shared__ u32 cnt[];                           // 2^bb counters
    const u32 N_BINS = 1u << bb;
    if (blockIdx.x >= *n_work) return;                     // (the grid is the list's upper bound: its length never visits the host)
    const CountWork wk = work[blockIdx.x];
    const u32 b = wk.bucket, lane = threadIdx.x & 63u;
    const u32 start = wk.start, end = wk.end;
    for (u32 q = threadIdx.x; q < N_BINS; q += TPB_COUNT) cnt[q] = 0;
    __syncthreads();
    // one element for every lane of the wave (wave-uniform call: the ballots).  A hot EC fills most lanes of a wave: it is added
    // once per wave, the rest go one by one.
    auto add = [&](u32 bin, bool have) {
        const u64 hm = __ballot(have);
        if (!hm) return;
        const u32 v = (u32)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)hm) - 1);      // (the lane index is wave-uniform: a VALU readlane, not __shfl's trip through the LDS crossbar)
        const bool same = have && bin == v;
        const u64 m = __ballot(same);
        if (__popcll(m) >= 8) {
            if (lane == (u32)(__ffsll((long long)m) - 1)) atomicAdd(&cnt[v], (u32)__popcll(m));
            if (have && !same) atomicAdd(&cnt[bin], 1u);
        } else if (have) {
            atomicAdd(&cnt[bin], 1u);
        }
    };
    // 16 bytes = 8 elements per lane and load where the piece allows, four loads in flight; its ragged ends one element per thread
    const u32 a0 = min((start + 7u) & ~7u, end), a1 = max(end & ~7u, a0);
    { const u32 i = start + threadIdx.x; const bool have = i < a0; add(have ? (u32)pairs[i] : 0u, have); }
    { const u32 i = a1 + threadIdx.x; const bool have = i < end; add(have ? (u32)pairs[i] : 0u, have); }
    for (u32 i0 = a0; i0 < a1; i0 += 32 * TPB_COUNT) {
        uint4 pv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 i = i0 + (k * TPB_COUNT + threadIdx.x) * 8u;
            pv[k] = i < a1 ? *reinterpret_cast<const uint4*>(pairs + i) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool have = i0 + (k * TPB_COUNT + threadIdx.x) * 8u < a1;
            const u32 w[4] = {pv[k].x, pv[k].y, pv[k].z, pv[k].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) add((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu, have);
        }
    }
    __syncthreads();
    // Every EC of a handle that has only seen its own reads has at least one read: the slots this workgroup adds a count to are
    // exactly the occupied slots of its range, and the first to add to a slot (counts start at zero) puts it on the list of
    // occupied slots, with its first read and key length, and marks that read in the first-appearance bitmap -- the slot's line
    // is in hand here.  finalize then needs no pass over the table (1 GB at 2^24 slots) to find 3.7 M entries.
    // A whole range with a sink (the usual case) visits every occupied slot's line ONCE: how many there are is known from the LDS
    // counters alone, so the list positions are handed out first, and then one look at the slot's line (n1, off, count,
    // first_inv) serves the count update, the list entry and the bitmap -- eight slots' loads in flight per thread.
    const bool once = sink.list && !wk.shared;
    u32 mine = 0;
    for (u32 q = threadIdx.x; q < N_BINS; q += TPB_COUNT) {
        const u32 c = cnt[q];
        u32 first = 0;
        if (once) first = c != 0u;
        else if (c) {
            Slot* s = table + (((u64)b << bb) | q);
            if (wk.shared) first = atomicAdd(&s->count, c) == 0u;
            else { s->count += c; first = 1u; }             // the only writer of its slots
        }
        if (sink.list && !once) cnt[q] = first;
        mine += first;
    }
    if (!sink.list) return;
    __shared__ u32 s_wtot[TPB_COUNT / 64];
    __shared__ u64 s_base;
    const u32 incl = wave_incl_scan(mine);
    if (lane == 63) s_wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int k = 0; k < TPB_COUNT / 64; ++k) { const u32 c = s_wtot[k]; s_wtot[k] = run; run += c; }
        s_base = run ? atomicAdd(sink.n_list, (u64)run) : 0ull;
    }
    __syncthreads();
    u64 at = s_base + s_wtot[threadIdx.x >> 6] + (incl - mine);
    if (once) {
        for (u32 q0 = threadIdx.x; q0 < N_BINS; q0 += 8 * TPB_COUNT) {
            u32 c[8];
            uint2 vk[8], vc[8];                              // {n1, off} and {count, first_inv}: two 8-byte words of the slot's line
#pragma unroll
            for (int k = 0; k < 8; ++k) { const u32 q = q0 + k * TPB_COUNT; c[k] = q < N_BINS ? cnt[q] : 0u; }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c[k]) {
                    const Slot* sl = table + (((u64)b << bb) | (q0 + k * TPB_COUNT));
                    vk[k] = *reinterpret_cast<const uint2*>(&sl->n1); vc[k] = *reinterpret_cast<const uint2*>(&sl->count);
                }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!c[k]) continue;
                const u64 i = ((u64)b << bb) | (q0 + k * TPB_COUNT);
                table[i].count = vc[k].x + c[k];
                if (at < sink.max_list) {
                    sink.list[at] = (u32)i;
                    if (sink.list_fn) {
                        const u32 f = ~vc[k].y;
                        sink.list_fn[at] = make_uint2(f, vk[k].x - 1u);
                        if (f < sink.n_bits) atomicOr(&sink.bitmap[f >> 5], 1u << (f & 31u));
                    }
                }
                ++at;
            }
        }
        return;
    }
    for (u32 q = threadIdx.x; q < N_BINS; q += TPB_COUNT) {
        if (!cnt[q]) continue;
        const u64 i = ((u64)b << bb) | q;
        if (at < sink.max_list) {
            const Slot* s = table + i;
            sink.list[at] = (u32)i;
            if (sink.list_fn) {
                const u32 f = ~s->first_inv;
                sink.list_fn[at] = make_uint2(f, s->n1 - 1u);
                if (f < sink.n_bits) atomicOr(&sink.bitmap[f >> 5], 1u << (f & 31u));
            }
        }
        ++at;
    }
}

// ---------------------------------------------------------------------------------------------
// k_slow: one workgroup per deferred read (longer than a tile, or bounced off a full table).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_slow_len(const u32* rid, u64 n, const u64* queue, u64 nq, u64* len, u32 tw) {
    // length in records of each queued read (its head index .. the next change of read_id)
    const u64 q = blockIdx.x;
    if (q >= nq) return;
    __shared__ u64 s_end;
    const u64 h = queue[q];
    const u32 r0 = rid[rec_at(h, tw)];
    if (threadIdx.x == 0) s_end = n;
    __syncthreads();
    for (u64 b = h; b < n; b += TPB) {
        const u64 i = b + threadIdx.x;
        if (i < n && rid[rec_at(i, tw)] != r0) atomicMin(&s_end, i);
        __syncthreads();
        const bool found = (s_end != n);
        __syncthreads();
        if (found) break;
    }
    __syncthreads();
    if (threadIdx.x == 0) len[q] = s_end - h;
}

struct SlowArgs {
    const u32* rid; const u32* loc; const u32* hf;
    const u64* queue; const u64* len; const u64* scr_off;   // per queued read
    u32* scr_key; u32* scr_mask;                            // global scratch tables (zeroed)
    u32 n_loci, n_haps;
    Slot* table; u64 cap_mask;
    uint2* arena; u64 arena_cap;
    Counters* ctr;
    u32* read_slot; u64 reads_hi;
    u64* requeue; u64* n_requeue;                           // reads that still found no slot
    u32 verify;                                             // exactness pass: compare with the read's EC instead of inserting
};

__device__ __forceinline__ u64 slow_probe_start(u32 lc, u64 cap2) { return __umul64hi((u64)(lc * 0x9E3779B1u) << 32, cap2); }

// The read's {locus -> mask} table (2 slots per record) sits in LDS when it fits SLOW_LDS slots (reads of up to 2 048 records:
// all but the pathological ones), in the global scratch otherwise: its compare-and-swaps are what a long read costs.
constexpr u32 SLOW_LDS = 4096;
// (IN_LDS is a template argument, not a pointer picked at run time: with one pointer for both homes every access to the read's table was a FLAT
//  instruction with agent-scope ordering -- compare-and-swaps, ORs and "atomic" loads on what is, for all but pathological reads, this workgroup's
//  own LDS.  profiles/r04_long_reads.txt)
template <bool IN_LDS> __device__ __forceinline__ u32 slow_ld(const u32* p) {
    if constexpr (IN_LDS) return *p; else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool IN_LDS>
__device__ __forceinline__ void slow_body(const SlowArgs& A, u32* key, u32* msk, const u64 q, const u64 h, const u64 L) {
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u64 cap2 = 2 * L;
    if (IN_LDS) {
        for (u32 p = tid; p < (u32)cap2; p += TPB) { key[p] = 0; msk[p] = 0; }
        __syncthreads();
    }
    __shared__ u64 s_acc[TPB / 64];
    __shared__ u32 s_n[TPB / 64];
    __shared__ u64 s_lo, s_j;
    __shared__ u32 s_np, s_st, s_n1, s_off, s_cnt, s_diff, s_inc, s_probes;

    for (u64 i = tid; i < L; i += TPB) {
        const u32 f = A.hf[rec_at(h + i, A_TW(A))];
        if (!rec_valid(f)) continue;
        const u32 lc = A.loc[rec_at(h + i, A_TW(A))], hap = (f >> ECB_HAP_SHIFT) & 0xFFu;
        if (lc >= A.n_loci || hap >= A.n_haps) { atomicOr(&A.ctr->err, ERR_RANGE); continue; }
        u64 p = slow_probe_start(lc, cap2);
        for (;;) {
            const u32 old = atomicCAS(&key[p], 0u, lc + 1u);
            if (old == 0u || old == lc + 1u) { atomicOr(&msk[p], 1u << hap); break; }
            if (++p == cap2) p = 0;
        }
    }
    if (!IN_LDS) __threadfence();
    __syncthreads();
    u64 a0 = 0;
    u32 np = 0;
    for (u64 p = tid; p < cap2; p += TPB) {
        const u32 k = slow_ld<IN_LDS>(&key[p]);
        if (k) {
            const u32 m = slow_ld<IN_LDS>(&msk[p]);
            ++np;
            a0 += pair_hash64(k - 1u, m);                   // same set hash as k_stream
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) a0 += __shfl_xor(a0, d);
    np = wave_sum(np);
    if (lane == 0) { s_acc[tid >> 6] = a0; s_n[tid >> 6] = np; }
    __syncthreads();
    const u32 r0 = A.rid[rec_at(h, A_TW(A))];
    if (tid == 0) {
        a0 = 0; np = 0;
        for (int w = 0; w < TPB / 64; ++w) { a0 += s_acc[w]; np += s_n[w]; }
        s_np = np; s_lo = finish_hash(a0, np); s_j = s_lo & A.cap_mask; s_probes = 0; s_cnt = 0;
        if ((u64)r0 >= A.reads_hi) { atomicOr(&A.ctr->err, ERR_CONTRACT); s_st = ST_NONE; }
        else s_st = ST_PENDING;
    }
    __syncthreads();
    np = s_np;
    // Is the key of slot s_j the set in the scratch table?  Thread 0 polls the slot's {n1, off} word; every thread takes
    // pairs tid, tid + TPB, ... with fresh reads (the slot may be in the middle of being published by another CU: a pair
    // whose mask is still zero sends everybody round again).  CMP_EQUAL / CMP_DIFFERENT, or CMP_INCOMPLETE = gave up.
    auto same_key = [&]() -> int {
        for (u32 spin = 0; spin < SPIN_MAX; ++spin) {
            __syncthreads();
            if (tid == 0) {
                const u64 w = fresh64(reinterpret_cast<u64*>(&A.table[s_j].n1));
                s_n1 = (u32)w; s_off = (u32)(w >> 32); s_diff = 0; s_inc = 0;
            }
            __syncthreads();
            const u32 n1 = s_n1;
            if (n1 == DEAD_KEY) return CMP_DIFFERENT;
            if (n1 == 0u) { __builtin_amdgcn_s_sleep(8); continue; }
            const u32 n = n1 - 1u;
            if (n != np) return CMP_DIFFERENT;
            Slot* sl = A.table + s_j;
            bool diff = false, inc = false;
            for (u32 i = tid; i < n && !diff && !inc; i += TPB) {
                u64* src = reinterpret_cast<u64*>(i < INL ? &sl->pair[i] : A.arena + ((u64)s_off + (i - INL)));
                // (a pair only ever goes from zero to its final value: a plain load that shows a mask shows the pair; only a zero is
                //  asked again where no cache can answer -- a key of 700 pairs was 700 read-modify-writes per compare)
                uint2 pr = unpack2(*src);
                if (pr.y == 0u) pr = unpack2(fresh64(src));
                if (pr.y == 0u) { inc = true; break; }
                diff = true;
                if (pr.x < A.n_loci) {
                    u64 p = slow_probe_start(pr.x, cap2);
                    for (u64 t = 0; t < cap2; ++t) {
                        const u32 k = slow_ld<IN_LDS>(&key[p]);
                        if (k == pr.x + 1u) { diff = slow_ld<IN_LDS>(&msk[p]) != pr.y; break; }
                        if (k == 0u) break;
                        if (++p == cap2) p = 0;
                    }
                }
            }
            if (diff) atomicOr(&s_diff, 1u);
            if (inc) atomicOr(&s_inc, 1u);
            __syncthreads();
            if (s_diff) return CMP_DIFFERENT;                     // (a complete pair that is not mine settles it, whatever is still missing)
            if (!s_inc) return CMP_EQUAL;
            __builtin_amdgcn_s_sleep(8);
        }
        return CMP_INCOMPLETE;
    };
    if (A.verify) {
        if (s_st != ST_NONE) {
            if (tid == 0) s_j = A.read_slot[r0];
            __syncthreads();
            const bool same = s_j != (u64)PENDING && same_key() == CMP_EQUAL;
            if (tid == 0 && !same) atomicAdd(&A.ctr->n_mismatch, 1ull);
        }
    } else {
        // find or insert, one probe sequence driven by thread 0, key compares by the whole workgroup
        for (u32 round = 0; round < 4 * MAX_PROBE && s_st == ST_PENDING; ++round) {
            __syncthreads();
            if (tid == 0) {
                u64 j = s_j; u32 probes = s_probes;
                struct Defer { __device__ int quick(const SlotView&) const { return CMP_UNSURE; } };   // ST_PENDING = "slot j carries my hash": compared below
                const int st = table_lookup(A.table, A.cap_mask, s_lo, j, probes, Defer());
                s_j = j; s_probes = probes; s_st = (u32)st; s_off = 0; s_n1 = 0;
                if (st == ST_CREATED) {
                    u64 off = 0;
                    if (np > INL) off = arena_alloc(A.ctr, A.arena_cap, np - INL, blockIdx.x);
                    atomicAdd(&A.ctr->n_ecs, 1ull);
                    s_off = (u32)off;
                    if (off == ~0ull) { atomicOr(&A.ctr->err, ERR_ARENA); s_n1 = DEAD_KEY; }
                } else if (st == ST_FULL) {
                    A.requeue[atomicAdd(A.n_requeue, 1ull)] = h;
                }
            }
            __syncthreads();
            if (s_st == ST_PENDING) {
                const int r = same_key();
                __syncthreads();
                if (tid == 0) {
                    RACE(2);
                    if (r == CMP_DIFFERENT) RACE(3);
                    if (r == CMP_EQUAL) { s_st = ST_HIT; A.read_slot[r0] = (u32)s_j; atomicMax(&A.table[s_j].first_inv, ~r0); }
                    else if (r == CMP_INCOMPLETE) { s_st = ST_NONE; atomicOr(&A.ctr->err, ERR_INTERNAL); }
                    else { s_j = (s_j + 1) & A.cap_mask; s_probes += 1; if (s_probes >= MAX_PROBE) { s_st = ST_FULL; A.requeue[atomicAdd(A.n_requeue, 1ull)] = h; } }
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if (s_st == ST_CREATED) {                           // publish: pairs (write-through) by everybody, {n1, off} by one; no waiting
            Slot* sl = A.table + s_j;
            const bool dead = s_n1 == DEAD_KEY;
            if (!dead) for (u64 p = tid; p < cap2; p += TPB) {
                const u32 k = slow_ld<IN_LDS>(&key[p]);
                if (k) {
                    const u32 m = slow_ld<IN_LDS>(&msk[p]);
                    const u32 pos = atomicAdd(&s_cnt, 1u);
                    uint2* dst = pos < INL ? &sl->pair[pos] : A.arena + ((u64)s_off + (pos - INL));
                    store_wt64(reinterpret_cast<u64*>(dst), pack2(make_uint2(k - 1u, m)));
                }
            }
            if (tid == 0) {
                publish_key(sl, dead ? DEAD_KEY : np + 1u, s_off);
                A.read_slot[r0] = (u32)s_j;
                atomicMax(&sl->first_inv, ~r0);
            }
        }
    }
    __syncthreads();
    if (!IN_LDS) for (u64 p = tid; p < cap2; p += TPB) {    // leave the global scratch zeroed for the next round
        if (slow_ld<IN_LDS>(&key[p])) { key[p] = 0; msk[p] = 0; }
    }
}
__global__ __launch_bounds__(TPB) void k_slow(SlowArgs A) {
    extern __shared__ u32 sh_scr[];                // SLOW_LDS keys, SLOW_LDS masks
    const u64 q = blockIdx.x;
    const u64 h = A.queue[q], L = A.len[q];
    if (2 * L <= (u64)SLOW_LDS) slow_body<true>(A, sh_scr, sh_scr + SLOW_LDS, q, h, L);
    else slow_body<false>(A, A.scr_key + A.scr_off[q], A.scr_mask + A.scr_off[q], q, h, L);
}

// ---------------------------------------------------------------------------------------------
// table maintenance: grow (rehash), compact, merge
// ---------------------------------------------------------------------------------------------
// new_of_old[i] = where slot i went: the reads' slot ids are re-mapped through it (no second lookup, no hashing)
__global__ void k_rehash(const Slot* old_t, u64 old_cap, Slot* new_t, u64 new_mask, u32* new_of_old) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < old_cap; i += (u64)gridDim.x * blockDim.x) {
        const Slot s = old_t[i];
        if (!s.n1) continue;
        u64 j = s.lo & new_mask;
        for (;; j = (j + 1) & new_mask) {                // the new table is larger; two ECs with one hash take two slots
            if (atomicCAS(&new_t[j].lo, 0ull, s.lo) == 0ull) {
                Slot t = s;
                uint4* d = reinterpret_cast<uint4*>(new_t + j);
                const uint4* v = reinterpret_cast<const uint4*>(&t);
                d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
                new_t[j].off = s.off; new_t[j].n1 = s.n1;
                new_of_old[i] = (u32)j;
                break;
            }
        }
    }
}

__global__ void k_remap_read_slot(u32* read_slot, u64 n_reads, const u32* new_of_old) {
    for (u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x; r < n_reads; r += (u64)gridDim.x * blockDim.x) {
        const u32 os = read_slot[r];
        if (os != PENDING) read_slot[r] = new_of_old[os];
    }
}

// occupied slots -> dense list (order irrelevant: ranks come from `first`); one global atomic per 4096 slots
constexpr int TPB_COMPACT = 1024;
// (finalize passes bitmap / list_fn: the slot being scanned already holds the EC's first read and key length, so the
//  first-appearance bitmap is marked and both are written next to the list here -- coalesced -- instead of being gathered
//  from the table again by separate kernels)
__global__ __launch_bounds__(TPB_COMPACT) void k_compact(const Slot* table, u64 cap, u32* list, u64 max_list, u64* n_list,
                                                         u32* bitmap, u64 n_bits, uint2* list_fn) {
    __shared__ u32 s_w[TPB_COMPACT / 64];
    __shared__ u64 s_base;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    for (u64 b = (u64)blockIdx.x * 4 * TPB_COMPACT; b < cap; b += (u64)gridDim.x * 4 * TPB_COMPACT) {
        u32 occ = 0, off[4], tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 i = b + (u64)k * TPB_COMPACT + tid;
            const bool o = i < cap && table[i].n1 != 0u;
            const u64 m = __ballot(o);
            off[k] = tot + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
            tot += (u32)__popcll(m);
            occ |= (u32)o << k;
        }
        if (lane == 0) s_w[w] = tot;
        __syncthreads();
        if (tid == 0) {
            u32 run = 0;
            for (int k = 0; k < TPB_COMPACT / 64; ++k) { const u32 c = s_w[k]; s_w[k] = run; run += c; }
            s_base = run ? atomicAdd(n_list, (u64)run) : 0ull;
        }
        __syncthreads();
        const u64 base = s_base + s_w[w];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((occ >> k & 1u) && base + off[k] < max_list) {
                const u64 i = b + (u64)k * TPB_COMPACT + tid;
                list[base + off[k]] = (u32)i;
                if (list_fn) {
                    const u32 f = ~table[i].first_inv;
                    list_fn[base + off[k]] = make_uint2(f, table[i].n1 - 1u);
                    if (f < n_bits) atomicOr(&bitmap[f >> 5], 1u << (f & 31u));
                }
            }
        __syncthreads();
    }
}

// ... and with the list already there (a merged table that kept it): what k_compact writes next to the list, from the list
__global__ void k_list_fn(const Slot* table, const u32* list, u64 max_list, const u64* n_list, u64* n_out, u32* bitmap, u64 n_bits, uint2* list_fn) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const u64 n = *n_list;
    if (e == 0) *n_out = n;
    if (e >= n || e >= max_list) return;
    const Slot* s = table + list[e];
    const u32 f = ~s->first_inv;
    list_fn[e] = make_uint2(f, s->n1 - 1u);
    if (f < n_bits) atomicOr(&bitmap[f >> 5], 1u << (f & 31u));
}

// Partitioned export (multi-GPU merge by key range): part of an EC = a few high bits of its key, so every rank sends
// part p of its table to rank p, rank p merges what it gets, and no EC is ever merged on two ranks.
constexpr u32 MAX_PARTS = 64;
__device__ __forceinline__ u32 part_of(u64 lo, u32 n_parts) { return (u32)((lo >> 40) % n_parts); }   // (the low bits pick the table slot)

constexpr u32 PARTS_PER_BLOCK = 16 * TPB;     // entries per workgroup: same-address global atomics cost ~50 ns each, so few of them
__global__ __launch_bounds__(TPB) void k_parts_count(const Slot* table, const u32* list, u64 n, u32 n_parts, u64* cnt) {
    __shared__ u32 ce[MAX_PARTS], cp[MAX_PARTS];
    if (threadIdx.x < MAX_PARTS) { ce[threadIdx.x] = 0; cp[threadIdx.x] = 0; }
    __syncthreads();
    const u64 e0 = blockIdx.x * (u64)PARTS_PER_BLOCK, e1 = min(e0 + PARTS_PER_BLOCK, n);
    for (u64 eb = e0; eb < e1; eb += TPB) {
        const u64 e = eb + threadIdx.x;
        u32 q = MAX_PARTS, np = 0;
        if (e < e1) { const Slot& s = table[list[e]]; q = part_of(s.lo, n_parts); np = s.n1 - 1u; }
        for (u32 t = 0; t < n_parts; ++t) {          // one LDS atomic per wave and part (few parts = few, hot counters)
            const u64 m = __ballot(q == t);
            if (!m) continue;
            const u32 tot = wave_sum(q == t ? np : 0u);
            if ((threadIdx.x & 63u) == 0) { atomicAdd(&ce[t], (u32)__popcll(m)); atomicAdd(&cp[t], tot); }
        }
    }
    __syncthreads();
    if (threadIdx.x < n_parts) {
        if (ce[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (u64)ce[threadIdx.x]);
        if (cp[threadIdx.x]) atomicAdd(&cnt[n_parts + threadIdx.x], (u64)cp[threadIdx.x]);
    }
}
// cur[0..n_parts) / cur[n_parts..2 n_parts): next free entry / pair of every part (start = the part's offset);
// pair_base[q] = first pair of part q: Entry::off is written relative to it.  Two walks over the workgroup's entries:
// count per part, reserve (one global atomic per part), then place.  Keys leave SORTED by locus (ranked like the CSR rows
// of k_emit_*): two exported keys are then equal iff they are equal element by element, which is what k_merge tests first.
// Keys of more than EXPORT_SMALL pairs are queued for k_parts_sort_big (one wave each).
constexpr u32 EXPORT_SMALL = RANKED_MAX;
__global__ __launch_bounds__(TPB) void k_parts_export(const Slot* table, const u32* list, u64 n, const uint2* arena, u32 n_parts,
                                                      u64* cur, const u64* pair_base, Entry* out_e, uint2* out_p, u32 read_base,
                                                      u64* big, u32* n_big) {
    __shared__ u32 ce[MAX_PARTS], cp[MAX_PARTS];
    __shared__ u64 be[MAX_PARTS], bp[MAX_PARTS];
    const u32 lane = threadIdx.x & 63u;
    const u64 e0 = blockIdx.x * (u64)PARTS_PER_BLOCK, e1 = min(e0 + PARTS_PER_BLOCK, n);
    for (int pass = 0; pass < 2; ++pass) {
        if (threadIdx.x < MAX_PARTS) { ce[threadIdx.x] = 0; cp[threadIdx.x] = 0; }
        __syncthreads();
        for (u64 eb = e0; eb < e1; eb += TPB) {
            const u64 e = eb + threadIdx.x;
            uint4 sa = make_uint4(0u, 0u, 1u, 0u), sb = sa, sc = sa, sd = sa;      // the slot's line (n1 = 1: an empty key)
            u32 q = MAX_PARTS, re = 0, rp = 0, sn = 0;
            if (e < e1) {
                const uint4* sl = reinterpret_cast<const uint4*>(table + list[e]);
                sa = sl[0]; sb = sl[1]; sc = sl[2]; sd = sl[3];
                q = part_of(((u64)sa.y << 32) | sa.x, n_parts); sn = sa.z - 1u;
            }
            for (u32 t = 0; t < n_parts; ++t) {      // rank within the workgroup: wave prefix + one LDS atomic per wave and part
                const bool mine = q == t;
                const u64 m = __ballot(mine);
                if (!m) continue;
                const u32 v = mine ? sn : 0u, incl = wave_incl_scan(v);
                const u32 tot = (u32)__builtin_amdgcn_readlane((int)incl, 63);   // (read here, with every lane alive: inside the branch below
                u32 b_e = 0, b_p = 0;                                            //  the compiler sinks the scan's last add under exec = lane 0)
                if (lane == 0) { b_e = atomicAdd(&ce[t], (u32)__popcll(m)); b_p = atomicAdd(&cp[t], tot); }
                b_e = (u32)__builtin_amdgcn_readfirstlane((int)b_e); b_p = (u32)__builtin_amdgcn_readfirstlane((int)b_p);
                if (mine) { re = b_e + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u)); rp = b_p + incl - v; }
            }
            if (pass == 1 && e < e1) {
                const u64 po = bp[q] + rp;
                if (sn <= EXPORT_SMALL) {
                    ranked_pairs(make_view(sa, sb, sc, sd), arena, [&](u32 r, u32 x, u32 y) { out_p[po + r] = make_uint2(x, y); });
                } else {
                    const u32 bi = atomicAdd(n_big, 1u);
                    big[2 * (u64)bi] = po; big[2 * (u64)bi + 1] = ((u64)list[e] << 32) | sn;
                }
                Entry en;
                en.lo = ((u64)sa.y << 32) | sa.x; en.reserved = 0; en.count = sb.x;
                en.first_inv = ~(~sb.y + read_base);
                en.off = (u32)(po - pair_base[q]); en.n = sn;
                out_e[be[q] + re] = en;
            }
        }
        __syncthreads();
        if (pass == 0 && threadIdx.x < n_parts) {
            be[threadIdx.x] = ce[threadIdx.x] ? atomicAdd(&cur[threadIdx.x], (u64)ce[threadIdx.x]) : 0ull;
            bp[threadIdx.x] = cp[threadIdx.x] ? atomicAdd(&cur[n_parts + threadIdx.x], (u64)cp[threadIdx.x]) : 0ull;
        }
        __syncthreads();
    }
}
// long keys of an export: one wave per key, rank = number of smaller loci
__global__ __launch_bounds__(TPB) void k_parts_sort_big(const Slot* table, const uint2* arena, const u64* big, u32 n_big, uint2* out_p) {
    __shared__ __attribute__((aligned(16))) u32 sx[TPB / 64][BIG_LDS];
    const u32 b = (blockIdx.x * TPB + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (b >= n_big) return;
    const u64 po = big[2 * (u64)b];
    const u32 n = (u32)big[2 * (u64)b + 1];
    const Slot& s = table[big[2 * (u64)b + 1] >> 32];
    ranked_pairs_wave(s, arena, n, sx[threadIdx.x >> 6], lane, [&](u32 r, u32 x, u32 y) { out_p[po + r] = make_uint2(x, y); });
}
// adopt: entries known to be distinct ECs go to consecutive slots of an empty table, no hashing.  The pair list was copied to
// the arena at arena_base as it is: the slot takes its first INL pairs, the rest stay where they are.
__global__ void k_adopt(const Entry* ent, u64 n, const uint2* pairs, Slot* table, u64 slot_base, u32 arena_base) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const Entry en = ent[e];
    Slot s{};
    s.lo = en.lo; s.n1 = en.n + 1u; s.off = arena_base + en.off + INL; s.count = en.count; s.first_inv = en.first_inv;
    for (u32 i = 0; i < INL && i < en.n; ++i) s.pair[i] = pairs[(u64)en.off + i];
    table[slot_base + e] = s;
}

// The ordered merge of bam_utils.py:680-724, one thread per incoming EC: find its key in the table (exact compare) or
// insert it; counts are added, first appearances minimised.
struct ListCmp {                                   // incoming key = a sorted pair list; stored key = slot + arena, read fresh
    const uint2* inc; u32 n; uint2* arena;
    __device__ __forceinline__ int quick(const SlotView& v) const { return v.n != n ? CMP_DIFFERENT : CMP_UNSURE; }   // (keys are compared in full(): not a hot path)
    __device__ __noinline__ int full(Slot* s, u32 sn, u32 off) const {
        if (sn != n) return CMP_DIFFERENT;
        bool same = true, inc_ = false;            // both sorted (keys that came from an export): element by element
        for (u32 i = 0; i < n && same; ++i) {
            const uint2 a = key_pair_fresh(s, arena, off, i), b = inc[i];
            inc_ |= a.y == 0u;
            same = a.x == b.x && a.y == b.y;
        }
        if (same) return CMP_EQUAL;
        if (inc_) return CMP_INCOMPLETE;
        for (u32 i = 0; i < n; ++i) {              // the stored key may be one k_stream wrote, in no order: compare as sets
            const uint2 a = key_pair_fresh(s, arena, off, i);
            if (a.y == 0u) return CMP_INCOMPLETE;
            bool found = false;
            for (u32 k = 0; k < n && !found; ++k) found = inc[k].x == a.x && inc[k].y == a.y;
            if (!found) return CMP_DIFFERENT;
        }
        return CMP_EQUAL;
    }
};
constexpr u32 MERGE_PER_BLOCK = 2 * TPB;      // entries per workgroup: a piece of one key range is a few hundred thousand entries, and with 16 x TPB
                                              // each it occupied 71 of the 256 CUs (one EC-count atomic per workgroup, fire and forget)
// All tables of a call in ONE launch (blockIdx.y = table): counts add and first reads minimise in any order, and a key that
// two tables bring at the same moment is settled by the publication protocol like two waves of k_stream founding one EC --
// eight pieces of a key range one after the other were eight launches of 0.04 ms that each left most of the chip idle.
struct MergeDesc { const Entry* ent; const uint2* pairs; u64 n, n_pairs; };
// (list / n_list, optional: every slot this launch founds is appended -- a table that started empty, or whose list of occupied
//  slots was current, keeps a current list, and neither an export nor finalize has to scan it for its few occupied slots)
__global__ __launch_bounds__(TPB) void k_merge(const MergeDesc* D, Slot* table, u64 cap_mask, uint2* arena, u64 arena_cap, Counters* ctr,
                                               u32* list, u64 list_cap, u64* n_list) {
    const MergeDesc d = D[blockIdx.y];
    const Entry* const ent = d.ent; const uint2* const pairs = d.pairs;
    const u64 n = d.n, n_pairs = d.n_pairs;
    if (blockIdx.x * (u64)MERGE_PER_BLOCK >= n) return;       // (the grid is as wide as the longest table)
    __shared__ u32 s_new;
    __shared__ u32 s_found[MERGE_PER_BLOCK];                  // the slots this workgroup founds (for `list`: one reservation per workgroup)
    __shared__ u32 s_nfound;
    __shared__ u64 s_lbase;
    if (threadIdx.x == 0) { s_new = 0; s_nfound = 0; }
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    const u64 e0 = blockIdx.x * (u64)MERGE_PER_BLOCK, e1 = min(e0 + MERGE_PER_BLOCK, n);
    u32 my_new = 0;                                // (wave-uniform)
    for (u64 eb = e0; eb < e1; eb += TPB) {
        const u64 e = eb + threadIdx.x;
        const bool on = e < e1;
        Entry s{};
        if (on) s = ent[e];
        const bool ok = on && (u64)s.off + s.n <= n_pairs && s.lo != 0ull;
        if (on && !ok) atomicOr(&ctr->err, ERR_CONTRACT);
        ListCmp cmp{pairs + s.off, s.n, arena};
        u64 j = s.lo & cap_mask;
        u32 probes = 0;
        int st = ST_NONE;
        if (ok) st = table_lookup(table, cap_mask, s.lo, j, probes, cmp);
        bool created = false;
        for (u32 round = 0;; ++round) {            // publish, then settle: as in k_stream (the creator a lane waits for may be its neighbour)
            const u64 cm = __ballot(st == ST_CREATED);
            if (cm) {
                const bool cr = st == ST_CREATED;
                const u32 want = cr && s.n > INL ? s.n - INL : 0u;
                u64 at = 0;
                if (__ballot(want != 0u)) {                                 // key arena: one reservation per wave, not per created EC
                    const u32 incl = wave_incl_scan(want);
                    const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                    if (lane == 0) at = arena_alloc(ctr, arena_cap, total, (blockIdx.y * gridDim.x + blockIdx.x) * (TPB / 64) + (threadIdx.x >> 6));
                    at = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(at >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)at);
                    if (at == ~0ull) { if (lane == 0) atomicOr(&ctr->err, ERR_ARENA); }
                    else at += incl - want;
                }
                my_new += (u32)__popcll(cm);
                if (list) {                                                 // (uniform; every entry founds at most one slot)
                    const int first = __ffsll((long long)cm) - 1;
                    u32 lb = 0;
                    if ((int)lane == first) lb = atomicAdd(&s_nfound, (u32)__popcll(cm));
                    lb = (u32)__builtin_amdgcn_readlane((int)lb, first);
                    if (cr) s_found[lb + __builtin_amdgcn_mbcnt_hi((u32)(cm >> 32), __builtin_amdgcn_mbcnt_lo((u32)cm, 0u))] = (u32)j;
                }
                if (cr) {
                    const bool dead = at == ~0ull;
                    if (!dead)
                        for (u32 t = 0; t < s.n; ++t) {
                            uint2* dst = t < INL ? &table[j].pair[t] : arena + (at + (t - INL));
                            store_wt64(reinterpret_cast<u64*>(dst), pack2(pairs[(u64)s.off + t]));
                        }
                    publish_key(table + j, dead ? DEAD_KEY : s.n + 1u, (u32)at);
                    st = ST_HIT; created = true;
                }
            }
            if (!__ballot(st == ST_PENDING)) break;
            if (round >= 64u) { if (st == ST_PENDING) { atomicOr(&ctr->err, ERR_INTERNAL); st = ST_NONE; } break; }
            if (st == ST_PENDING) {
                const int r = table_settle(table + j, cmp);
                RACE(2);
                if (r == ST_OTHER) RACE(3);
                if (r == ST_HIT) st = ST_HIT;
                else if (r == ST_STUCK) { atomicOr(&ctr->err, ERR_INTERNAL); st = ST_NONE; }
                else { j = (j + 1) & cap_mask; ++probes; st = table_lookup(table, cap_mask, s.lo, j, probes, cmp); }
            }
        }
        (void)created;
        if (st == ST_FULL) atomicAdd(&ctr->n_queue, 1ull);             // host sizes the table so this cannot happen
        else if (st == ST_HIT) {
            atomicAdd(&table[j].count, s.count);                      // one pair of atomics per merged EC, not per read
            atomicMax(&table[j].first_inv, s.first_inv);
        }
    }
    if (lane == 0 && my_new) atomicAdd(&s_new, my_new);
    __syncthreads();
    if (threadIdx.x == 0 && s_new) atomicAdd(&ctr->n_ecs, (u64)s_new);
    if (list) {
        if (threadIdx.x == 0) s_lbase = s_nfound ? atomicAdd(n_list, (u64)s_nfound) : 0ull;
        __syncthreads();
        for (u32 i = threadIdx.x; i < s_nfound; i += TPB) if (s_lbase + i < list_cap) list[s_lbase + i] = s_found[i];
    }
}

// ---------------------------------------------------------------------------------------------
// finalize: rank by first appearance, CSR emit
// ---------------------------------------------------------------------------------------------
// First-appearance ranks: rank of read f among the marked reads = marked reads before f's 64-byte line of the bitmap (an exclusive scan of the
// lines' popcounts: 1/16 of the bitmap's words, a table that stays in L2) + the marked bits before f within its line.  (A prefix per 32-bit word
// made every rank two reads of lines that are nowhere near each other -- the bitmap's and the prefix array's -- where this is one.)
constexpr u32 BM_LINE = 16;                     // bitmap words per line; the bitmap is allocated in whole lines (bitmap_words)
inline u64 bitmap_words(u64 n_bits) { return ((n_bits + 31) / 32 + BM_LINE) / BM_LINE * BM_LINE; }
__global__ void k_popc(const u32* in, u64 n_lines, u32* out) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const uint4* q = reinterpret_cast<const uint4*>(in + i * BM_LINE);
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < (int)BM_LINE / 4; ++k) { const uint4 v = q[k]; c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
    out[i] = c;
}
__device__ __forceinline__ u32 bit_rank(const u32* bitmap, const u32* lprefix, u32 f) {
    const uint4* q = reinterpret_cast<const uint4*>(bitmap + ((f >> 5) & ~(BM_LINE - 1u)));
    const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    const u32 w[BM_LINE] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
    const u32 k = (f >> 5) & (BM_LINE - 1u), below = (1u << (f & 31u)) - 1u;
    u32 r = lprefix[f >> 9];
    static_assert(BM_LINE == 16, "f >> 9: 512 bits per line");
#pragma unroll
    for (u32 i = 0; i < BM_LINE; ++i) r += __popc(w[i] & (i < k ? 0xFFFFFFFFu : i == k ? below : 0u));
    return r;
}

// Exclusive scan of u32, ONE pass over the data: a workgroup takes the next stretch of 16 384 values (a ticket: stretches start in
// order), publishes its sum, and one of its waves walks back over the stretches before it, 64 status words per step, adding their
// sums up to the nearest one whose inclusive prefix is known -- decoupled look-back, as in the radix sort below.  A status word is
// 2 bits of state and a 62-bit value, written and read with relaxed agent-scope atomics; the words and the ticket are zeroed by the
// launcher (scan_launch).  (Rounds 1-3a: per-block sums, a scan of the sums, per-block scan + offset -- three launches, the input read
// twice, and 4-byte loads at a 32-byte lane stride; 18 such scans were 1.4 ms of the config-4 path.)
// (stride: the input may be one member of an array of small structs -- element i is in[i * stride])
constexpr int SCB_TPB = 1024, SCB_ITEMS = 16, SCB = SCB_TPB * SCB_ITEMS;
constexpr u64 SC_AGG = 1ull << 62, SC_PFX = 2ull << 62, SC_VAL = (1ull << 62) - 1ull;
inline u64 scan_blocks(u64 n) { return std::max<u64>(1, (n + SCB - 1) / SCB); }
inline u64 scan_words(u64 n) { return 2 * (scan_blocks(n) + 2); }             // u32 words of scratch a scan of n values needs
__global__ __launch_bounds__(SCB_TPB) void k_scan_lb(const u32* in, u64 n, u32* out, u64* st, u64 nb, u64* d_total, u32 stride, u32* last32) {
    __shared__ u64 s_b, s_excl;
    __shared__ u32 s_w[SCB_TPB / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (tid == 0) s_b = atomicAdd(reinterpret_cast<unsigned long long*>(&st[nb]), 1ull);
    __syncthreads();
    const u64 b = s_b;
    if (b >= nb) return;
    const u64 base = b * SCB + (u64)tid * SCB_ITEMS;
    u32 v[SCB_ITEMS];
    const bool whole = base + SCB_ITEMS <= n;
    if (stride == 1u && whole && (reinterpret_cast<uintptr_t>(in) & 15u) == 0u) {
#pragma unroll
        for (int k = 0; k < SCB_ITEMS / 4; ++k) {
            const uint4 q = reinterpret_cast<const uint4*>(in + base)[k];
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCB_ITEMS; ++k) v[k] = base + k < n ? in[(base + k) * stride] : 0u;
    }
    u32 s = 0;
#pragma unroll
    for (int k = 0; k < SCB_ITEMS; ++k) s += v[k];
    const u32 incl = wave_incl_scan(s);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < SCB_TPB / 64; ++k) { const u32 c = s_w[k]; if (k < w) before += c; tot += c; }
    if (w == 0) {
        u64 excl = 0;
        if (lane == 0) __hip_atomic_store(&st[b], (b == 0 ? SC_PFX : SC_AGG) | (u64)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b > 0) {
            long long t = (long long)b - 1;                  // the nearest stretch not yet added
            for (u32 spins = 0; spins < (1u << 24);) {
                const long long idx = t - (long long)lane;
                const u64 x = idx >= 0 ? __hip_atomic_load(&st[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : SC_PFX;      // (before the first: prefix 0)
                const u64 ready = __ballot(x != 0ull), pfx = __ballot(x >= SC_PFX);
                u64 take = 0;                                // lanes whose value goes in
                if (pfx) {
                    const int p = __ffsll((long long)pfx) - 1;
                    const u64 need = p == 63 ? ~0ull : (1ull << (p + 1)) - 1ull;
                    if ((ready & need) == need) take = need;
                } else if (ready == ~0ull) take = ~0ull;
                if (!take) { ++spins; __builtin_amdgcn_s_sleep(1); continue; }
                u64 val = (take >> lane & 1ull) ? (x & SC_VAL) : 0ull;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) val += __shfl_xor(val, d);
                excl += val;
                if (pfx) break;
                t -= 64;
            }
            if (lane == 0) __hip_atomic_store(&st[b], SC_PFX | ((excl + tot) & SC_VAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_excl = excl;
            if (b + 1 == nb && d_total) *d_total = excl + tot;
            if (b + 1 == nb && last32) *last32 = (u32)(excl + tot);      // (a row-pointer array's last element: the total, where its scan ends)
        }
    }
    __syncthreads();
    u32 run = (u32)s_excl + before + incl - s;
    if (whole && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
#pragma unroll
        for (int k = 0; k < SCB_ITEMS / 4; ++k) {
            uint4 q;
            q.x = run; run += v[4 * k]; q.y = run; run += v[4 * k + 1]; q.z = run; run += v[4 * k + 2]; q.w = run; run += v[4 * k + 3];
            reinterpret_cast<uint4*>(out + base)[k] = q;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCB_ITEMS; ++k) { if (base + k < n) out[base + k] = run; run += v[k]; }
    }
}
// queue a scan on `st`: scratch = scan_words(n) u32 words (8-byte aligned); the total (64 bits) lands in *d_total (may be null)
inline hipError_t scan_launch(hipStream_t st, const u32* in, u64 n, u32* out, u32* scratch, u64* d_total, u32 stride = 1, u32* last32 = nullptr) {
    const u64 nb = scan_blocks(n);
    u64* words = reinterpret_cast<u64*>(scratch);
    hipError_t e = hipMemsetAsync(words, 0, ((nb + 1) * 8 + 15) & ~15ull, st);      // (nb + 1 words; in whole 16 bytes -- scan_words has the room --: the runtime fills a ragged end with a kernel of its own)
    if (e != hipSuccess) return e;
    k_scan_lb<<<(unsigned)nb, SCB_TPB, 0, st>>>(in, n, out, words, nb, d_total, stride, last32);
    return hipGetLastError();
}

// (slot and row length of rank r go out as one 8-byte word: the scatter is what this kernel costs, and two 4-byte stores to
//  two arrays were twice the partial lines; k_emit_small, which walks the ranks in order, writes `order` for the later readers)
__global__ void k_rank(const u32* list, const uint2* list_fn, u64 n, u64 n_bits, const u32* bitmap, const u32* wprefix,
                       uint2* ord2) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u32 si = list[e];
    const uint2 fn = list_fn[e];
    const u32 f = fn.x;
    if (f >= n_bits) return;                       // (an EC without a first read: finalize's count check reports it)
    const u32 r = bit_rank(bitmap, wprefix, f);
    if (r >= n) return;
    ord2[r] = make_uint2(si, fn.y);
}
// EC rank of every occupied slot: only the per-read EC ids need it (multisample, ecb_export_read_ec) -- a scatter over the
// whole table's index space that the single-sample result never reads
__global__ void k_slot_ranks(const u32* order, u64 n, u32* rank_of_slot) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r < n) rank_of_slot[order[r]] = (u32)r;
}

// CSR rows: every (locus, mask) pair of an EC is ranked by locus and written in place (columns ascending, as scipy's
// csc -> csr leaves them: bin_utils.py:211).  Short rows: one thread each.  Long rows: queued, one wave each.
// The indices the host supplied are validated here, once per EC instead of once per record.
constexpr u32 EMIT_SMALL = RANKED_MAX;
// The rows of a wave's 64 ECs are one stretch of `indices` / `data`: the ranked pairs are laid out in LDS and leave in whole lines (a lane
// storing its own row pair by pair wrote 4 bytes at a time, some twenty bytes apart from its neighbour's: three times the bytes in write
// transactions).  A wave with a long row among its 64 (k_emit_big's) stores directly.
__global__ __launch_bounds__(TPB) void k_emit_small(const Slot* table, const uint2* ord2, u32* order, u64 n, const uint2* arena,
                                                     const u32* indptr, int* indices, int* data, int* counts,
                                                     u32 n_loci, u32 n_haps, u32* big, u32* n_big, Counters* ctr) {
    __shared__ u32 sx[TPB / 64][64 * EMIT_SMALL], sy[TPB / 64][64 * EMIT_SMALL];
    const u64 e = (u64)blockIdx.x * TPB + threadIdx.x;
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool have = e < n;
    const u64 hm = __ballot(have);
    if (!hm) return;
    uint4 a = make_uint4(0u, 0u, 1u, 0u), b = a, c = a, d = a;      // (n1 = 1: an empty key)
    u32 dst = 0;
    if (have) {
        const u32 si = ord2[e].x;
        order[e] = si;
        const uint4* q = reinterpret_cast<const uint4*>(table + si);
        a = q[0]; b = q[1]; c = q[2]; d = q[3];
        counts[e] = (int)b.x;                       // Slot::count
        dst = indptr[e];
    }
    const SlotView v = make_view(a, b, c, d);
    const bool is_big = have && v.n > EMIT_SMALL;
    if (is_big) big[atomicAdd(n_big, 1u)] = (u32)e;
    const u32 base = (u32)__builtin_amdgcn_readfirstlane((int)dst);                                     // (lane 0 has an EC whenever any lane has)
    const u32 end = (u32)__builtin_amdgcn_readlane((int)(dst + v.n), 63 - __builtin_clzll(hm));        // ... and the last one that has ends the stretch
    const bool staged = __ballot(is_big) == 0ull && end - base <= 64u * EMIT_SMALL;
    bool bad = false;
    if (!is_big)
        ranked_pairs(v, arena, [&](u32 r, u32 x, u32 y) {
            if (staged) { const u32 at = min(dst - base + r, 64u * EMIT_SMALL - 1u); sx[w][at] = x; sy[w][at] = y; }     // (the bound: a broken row pointer must not reach beyond the stage)
            else { indices[dst + r] = (int)x; data[dst + r] = (int)y; }
            bad |= x >= n_loci || (y >> n_haps) != 0u;
        });
    if (staged) {
        wave_sync();
        for (u32 i = lane; i < end - base; i += 64u) { indices[base + i] = (int)sx[w][i]; data[base + i] = (int)sy[w][i]; }
    }
    if (bad) atomicOr(&ctr->err, ERR_RANGE);
}
__global__ __launch_bounds__(TPB) void k_emit_big(const Slot* table, const u32* order, const u32* big, const u32* n_big,
                                                   const uint2* arena, const u32* indptr, int* indices, int* data,
                                                   u32 n_loci, u32 n_haps, Counters* ctr) {
    __shared__ __attribute__((aligned(16))) u32 sx[TPB / 64][BIG_LDS];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nb = *n_big;
    bool bad = false;
    for (u32 b = (blockIdx.x * TPB + threadIdx.x) >> 6; b < nb; b += (gridDim.x * TPB) >> 6) {
        const u32 e = big[b];
        const Slot& s = table[order[e]];
        const u32 dst = indptr[e];
        ranked_pairs_wave(s, arena, s.n1 - 1u, sx[w], lane, [&](u32 r, u32 x, u32 y) {
            indices[dst + r] = (int)x;
            data[dst + r] = (int)y;
            bad |= x >= n_loci || (y >> n_haps) != 0u;
        });
    }
    if (bad) atomicOr(&ctr->err, ERR_RANGE);
}

// multisample: sort key = EC rank << 32 | (cell, file) of every read, the cell ABOVE the file: the triples come out in the order
// (EC, cell, file), in which the files of one (EC, cell) pair -- one entry of N -- follow each other
constexpr u32 MS_FILE_BITS = 32 - ECB_CELL_BITS;
__host__ __device__ __forceinline__ u32 ms_swz(u32 meta) { return ((meta & ((1u << ECB_CELL_BITS) - 1u)) << MS_FILE_BITS) | (meta >> ECB_CELL_BITS); }
__host__ __device__ __forceinline__ u32 ms_unswz(u32 s) { return (s >> MS_FILE_BITS) | (s << ECB_CELL_BITS); }
__host__ __device__ __forceinline__ u64 ms_swz_key(u64 key) { return (key & 0xFFFFFFFF00000000ull) | ms_swz((u32)key); }
__global__ void k_ms_keys(const u32* read_slot, const u32* rank_of_slot, const u32* meta, u64 n, u64* keys, u32* vals) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = ((u64)rank_of_slot[read_slot[i]] << 32) | ms_swz(meta[i]); vals[i] = (u32)i; }
}
__global__ void k_ms_swz_keys(u64* keys, u64 n) {           // EC << 32 | meta  ->  the sort key above, in place
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ms_swz_key(keys[i]);
}
// flag[i] = 1 where a run of equal sorted keys starts
__global__ void k_run_heads(const u64* keys, u64 n, u32* flag) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
__global__ void k_ms_emit(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u32 n_out,
                          u64* okey, u32* ofirst, u32* ostart) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n && flag[i]) { okey[pos[i]] = (keys[i] & 0xFFFFFFFF00000000ull) | ms_unswz((u32)keys[i]); ofirst[pos[i]] = vals[i]; ostart[pos[i]] = (u32)i; }
    if (i == 0) ostart[n_out] = (u32)n;
}
__global__ void k_ms_split(const u64* okey, const u32* ostart, const u32* ocount, u64 n, u32* ec, u32* meta, u32* count) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) { ec[i] = (u32)(okey[i] >> 32); meta[i] = (u32)okey[i]; count[i] = ocount ? ocount[i] : ostart[i + 1] - ostart[i]; }
}
// multisample across GPUs: the keys of the final ECs in rank order; their ranks looked up in a shard's own table; the
// shards' (EC, cell, file) triples combined on the root
__global__ void k_export_keys(const Slot* table, const u32* order, u64 n, u64* out) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e < n) out[e] = table[order[e]].lo;
}
// ... and where no table stands behind the result (it was assembled from per-range pieces): the hash of an EC is a function of its
// key alone -- the sum of its pairs' hashes, as the stream kernel forms it -- so it is taken from the finished CSR row
__global__ void k_row_keys(const u32* indptr, const int* indices, const int* data, u64 n, u64* out) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u32 a = indptr[e], z = indptr[e + 1];
    u64 acc = 0;
    for (u32 i = a; i < z; ++i) acc += pair_hash64((u32)indices[i], (u32)data[i]);
    out[e] = finish_hash(acc, z - a);
}
// EC e of the merged result = (hash keys[e], CSR row e with ascending loci).  Find it in this shard's table, by its hash and
// then by its key, pair for pair: grank[slot] = e.
__global__ void k_set_global_rank(const u64* keys, const int* indptr, const int* indices, const int* data, u64 n,
                                  const Slot* table, u64 cap_mask, const uint2* arena, u32* grank) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u64 lo = keys[e];
    const u32 r0 = (u32)indptr[e], rn = (u32)indptr[e + 1] - r0;
    u64 j = lo & cap_mask;
    for (u64 probe = 0; probe <= cap_mask; ++probe, j = (j + 1) & cap_mask) {
        const Slot& s = table[j];
        if (s.lo == 0ull) return;                                 // this shard never saw that EC
        if (s.lo != lo || s.n1 != rn + 1u) continue;
        bool same = true;
        for (u32 i = 0; i < rn && same; ++i) {
            const uint2 pr = key_pair(s, arena, i);
            u32 a = 0, b = rn;                                    // the row is sorted by locus
            while (a < b) { const u32 m = (a + b) >> 1; if ((u32)indices[r0 + m] < pr.x) a = m + 1; else b = m; }
            same = a < rn && (u32)indices[r0 + a] == pr.x && (u32)data[r0 + a] == pr.y;
        }
        if (same) { grank[j] = (u32)e; return; }
    }
}
__global__ void k_ms_out(const u64* okey, const u32* ofirst, const u32* ostart, u64 n, u32 read_base, u64* key, u32* count, u32* first) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) { key[i] = okey[i]; count[i] = ostart[i + 1] - ostart[i]; first[i] = ofirst[i] + read_base; }
}
__global__ void k_ms_combine(const u64* keys, const u32* idx, const u32* flag, const u32* pos, u64 n, const u32* cnt_in, const u32* first_in,
                             u64* okey, u32* ocount, u32* ofirst) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 o = pos[i] - (flag[i] ? 0u : 1u);                  // pos = exclusive scan of the head flags
    if (flag[i]) okey[o] = (keys[i] & 0xFFFFFFFF00000000ull) | ms_unswz((u32)keys[i]);
    atomicAdd(&ocount[o], cnt_in[idx[i]]);
    atomicMin(&ofirst[o], first_in[idx[i]]);
}


// ---------------------------------------------------------------------------------------------
// f-2: CSR(bitmask) <-> per-haplotype CSC (bin_utils.py:979-1028).  CSR -> CSC: a transposition of the non-zeros (k_cv_keys ...
// k_cv_ptr below).  CSC -> CSR: the set bits expanded to (row * T + column) keys, the stable radix sort (the LSD sort below),
// runs of equal keys OR-ed, row pointers by binary search on the sorted keys.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 lower_bound_u64(const u64* a, u64 n, u64 v) {
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}
// ---- per-haplotype CSC -> CSR(bitmask): a union per column, then a transposition ----------------------------------------------
//   k_cvu_colsum    S[l] = sum over haplotypes of their column pointers (S[l + 1] - S[l] row indices name column l); the pointers
//                   are checked here
//   k_cvu_pieces    a column is one piece of work, or -- above CVU_PIECE row indices -- several: equal ranges of EC ids
//   k_cvu_items / k_cvu_bounds   the list of pieces; where every haplotype's list of the column enters a piece's EC range
//                   (binary searches: lists of a column that is cut must be ascending, as scipy and the forward conversion write them)
//   k_cvu_union     one workgroup per piece: the piece's row indices from every haplotype's list go into an LDS hash
//                   {EC -> haplotype mask}; within a piece no order is needed and an EC listed twice ORs into the same bit.
//                   First launch: distinct ECs per column; second, behind a scan of those: the entries go out column by column as
//                   (EC << 32 | locus, mask) -- within a column in any order --
//   then a stable sort on the EC digits alone makes rows with ascending loci, and k_split_out / k_row_ptr write the CSR.
// A row index outside its piece's EC range (a cut column whose lists are not ascending) is noticed: the caller then takes the
// general, sort-everything path below.  A piece with more row indices than the table takes (EC ids bunched in one range) goes
// entry by entry: the first haplotype's copy of an EC gathers the mask by binary searches in the other haplotypes' lists.
constexpr u32 CVU_PIECE = 1536;     // row indices a piece aims at
constexpr u32 CVU_MAX = 3072;       // row indices the LDS table takes
constexpr u32 CVU_TSZ = 4096;       // table slots (a power of two; small pieces use a power-of-two part of it): 32 KB, four workgroups per CU
constexpr u32 CVU_TPB = 512;
constexpr u32 CVU_K = CVU_MAX / CVU_TPB;      // row indices per thread, all loaded before the first goes into the table
constexpr u32 CVB_ERR_PTR = 1u, CVB_ERR_EC = 2u, CVB_ERR_ORDER = 4u;
__global__ void k_cvb_last(const int* cscptr, u32 n_loci, u32 n_haps, int* last) {
    const u32 h = threadIdx.x;
    if (h < n_haps) last[h] = cscptr[(u64)h * (n_loci + 1) + n_loci];
}
__global__ void k_cvu_colsum(const int* cscptr, u32 n_loci, u32 n_haps, u32* S, u32* err) {
    const u64 l = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (l > n_loci) return;
    u32 sum = 0, bad = 0;
    for (u32 h = 0; h < n_haps; ++h) {
        const int* ptr = cscptr + (u64)h * (n_loci + 1);
        const int v = ptr[l];
        if (v < 0 || (l == 0 && v != 0) || (l > 0 && ptr[l - 1] > v)) bad = CVB_ERR_PTR;
        sum += (u32)v;
    }
    S[l] = sum;
    if (bad) atomicOr(err, bad);
}
__global__ void k_cvu_pieces(const u32* S, u32 n_loci, u32* pieces) {
    const u64 l = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (l >= n_loci) return;
    const u32 n = S[l + 1] - S[l];
    pieces[l] = n <= CVU_PIECE + CVU_PIECE / 2 ? (n ? 1u : 0u) : (n + CVU_PIECE - 1u) / CVU_PIECE;
}
__global__ void k_cvu_items(const u32* pieces, const u32* pbase, u32 n_loci, u32* item_col) {
    const u64 l = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (l >= n_loci) return;
    const u32 n = pieces[l], at = pbase[l];
    for (u32 r = 0; r < n; ++r) item_col[at + r] = (u32)l;
}
// EC range of piece r of a column cut into np pieces: [r * w, (r + 1) * w), w = ceil(n_ecs / np)
__device__ __forceinline__ u32 cvu_width(u32 n_ecs, u32 np) { return (u32)(((u64)n_ecs + np - 1u) / np); }
__global__ void k_cvu_bounds(const int* cscptr, const int* cscidx, const u64* hs, const u32* pieces, const u32* pbase, const u32* item_col,
                             u32 n_items, u32 n_loci, u32 n_haps, u32 n_ecs, u32* bnd) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= (u64)n_items * n_haps) return;
    const u32 i = (u32)(t / n_haps), h = (u32)(t % n_haps);
    const u32 l = item_col[i], np = pieces[l], r = i - pbase[l];
    const int* ptr = cscptr + (u64)h * (n_loci + 1);
    const u64 nh = hs[h + 1] - hs[h];
    u64 a = min((u64)(u32)ptr[l], nh), b = min((u64)(u32)ptr[l + 1], nh);
    if (r) {                                                 // first row index of the list at or above the piece's first EC
        const u64 lo = (u64)r * cvu_width(n_ecs, np);
        const int* base = cscidx + hs[h];
        while (a < b) { const u64 m = a + ((b - a) >> 1); if ((u64)(u32)base[m] < lo) a = m + 1; else b = m; }
    }
    bnd[t] = (u32)a;
}
// is EC e in haplotype hh's list of column l?  (lists ascending; a list that is not is reported and the answer discarded)
__device__ __forceinline__ bool cvb_contains(const int* cscptr, const int* cscidx, const u64* hs, u32 n_loci, u32 hh, u32 l, u32 e) {
    const int* p = cscptr + (u64)hh * (n_loci + 1);
    const u64 nh = hs[hh + 1] - hs[hh];
    u64 a = min((u64)(u32)p[l], nh), b = min((u64)(u32)p[l + 1], nh);
    const int* base = cscidx + hs[hh];
    while (a < b) { const u64 m = a + ((b - a) >> 1); const u32 v = (u32)base[m]; if (v < e) a = m + 1; else if (v > e) b = m; else return true; }
    return false;
}
template <bool EMIT>
__global__ __launch_bounds__(CVU_TPB) void k_cvu_union(const int* cscptr, const int* cscidx, const u64* hs, const u32* pieces, const u32* pbase,
                                                       const u32* item_col, const u32* bnd, u32 n_items, u32 n_loci, u32 n_haps, u32 n_ecs,
                                                       u32* colcnt, const u32* colbase, u32* colcur, u64 nnz, u64* keys, u32* vals, u32* err) {
    __shared__ u32 tkey[CVU_TSZ];
    __shared__ u32 tmask[CVU_TSZ];
    __shared__ u32 seg[64];                                  // per haplotype: first and one-past-last row index of the piece (within the haplotype)
    __shared__ u32 segp[33];                                 // ... and how many row indices the haplotypes before it bring
    __shared__ u64 shs[32];
    __shared__ u32 s_n, s_base;
    const u32 i = blockIdx.x;
    const u32 l = item_col[i], np = pieces[l], r = i - pbase[l];
    const u32 w = cvu_width(n_ecs, np);
    const u32 e_lo = (u32)min((u64)r * w, (u64)n_ecs), e_hi = r + 1u == np ? n_ecs : (u32)min((u64)(r + 1u) * w, (u64)n_ecs);
    if (threadIdx.x < n_haps) {
        const u32 h = threadIdx.x;
        const u64 h0 = hs[h], nh = hs[h + 1] - h0;
        shs[h] = h0;
        seg[2 * h] = bnd[(u64)i * n_haps + h];
        seg[2 * h + 1] = r + 1u < np ? bnd[(u64)(i + 1u) * n_haps + h] : (u32)min((u64)(u32)cscptr[(u64)h * (n_loci + 1) + l + 1], nh);
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (threadIdx.x == 0) { u32 run = 0; for (u32 h = 0; h < n_haps; ++h) { segp[h] = run; run += seg[2 * h + 1] - seg[2 * h]; } segp[n_haps] = run; }
    __syncthreads();
    const u32 tot = segp[n_haps];
    if (tot == 0) return;
    if (tot > CVU_MAX) {
        // entry by entry: the first haplotype's copy of an EC speaks for it
        for (u32 h = 0; h < n_haps; ++h) {
            const int* base = cscidx + hs[h];
            for (u32 j = seg[2 * h] + threadIdx.x; j < seg[2 * h + 1]; j += CVU_TPB) {
                const u32 e = (u32)base[j];
                u32 bad = e >= n_ecs ? CVB_ERR_EC : 0u;
                if (e < e_lo || e >= e_hi || (j > seg[2 * h] && (u32)base[j - 1] >= e)) bad |= CVB_ERR_ORDER;
                if (bad) { atomicOr(err, bad); continue; }
                bool first = true;
                for (u32 hh = h; hh-- > 0 && first;) first = !cvb_contains(cscptr, cscidx, hs, n_loci, hh, l, e);
                if (!first) continue;
                if (!EMIT) { atomicAdd(&colcnt[l], 1u); continue; }
                u32 mask = 1u << h;
                for (u32 hh = h + 1; hh < n_haps; ++hh) if (cvb_contains(cscptr, cscidx, hs, n_loci, hh, l, e)) mask |= 1u << hh;
                const u64 pos = (u64)colbase[l] + atomicAdd(&colcur[l], 1u);
                if (pos < nnz) { keys[pos] = ((u64)e << 32) | l; vals[pos] = mask; }
            }
        }
        return;
    }
    u32 tsz = 64;                                            // slots in use: a power of two, at least 4/3 of the row indices, at most the table
    while (tsz < CVU_TSZ && tsz < tot + tot / 3u + 1u) tsz <<= 1;      // (a piece of exactly CVU_MAX asks for 4 097: all 4 096 it gets, 3/4 full)
    static_assert(CVU_MAX < CVU_TSZ && (CVU_TSZ & (CVU_TSZ - 1u)) == 0, "a free slot is always found");
    // all of a thread's row indices are fetched before the first is inserted (their loads overlap), haplotype after haplotype in one index space
    u32 ev[CVU_K], hv[CVU_K];
#pragma unroll
    for (u32 k = 0; k < CVU_K; ++k) {
        const u32 u = threadIdx.x + k * CVU_TPB;
        hv[k] = 0xFFFFFFFFu; ev[k] = 0;
        if (u < tot) {
            u32 h = 0;
            while (segp[h + 1] <= u) ++h;
            hv[k] = h;
            ev[k] = (u32)cscidx[shs[h] + seg[2 * h] + (u - segp[h])];
        }
    }
    for (u32 q = threadIdx.x; q < tsz; q += CVU_TPB) { tkey[q] = 0xFFFFFFFFu; tmask[q] = 0u; }      // (while the loads are under way)
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < CVU_K; ++k) {
        if (hv[k] == 0xFFFFFFFFu) continue;
        const u32 e = ev[k];                                 // (never 0xFFFFFFFF once it is below n_ecs)
        if (e >= n_ecs) { atomicOr(err, CVB_ERR_EC); continue; }
        if (e < e_lo || e >= e_hi) { atomicOr(err, CVB_ERR_ORDER); continue; }
        u32 q = (e * 0x9E3779B1u) >> 7 & (tsz - 1u);
        for (u32 it = 0; it < tsz; ++it) {                   // (fewer keys than slots: a free one is always found)
            const u32 old = atomicCAS(&tkey[q], 0xFFFFFFFFu, e);
            if (old == 0xFFFFFFFFu || old == e) { atomicOr(&tmask[q], 1u << hv[k]); break; }
            q = (q + 1u) & (tsz - 1u);
        }
    }
    __syncthreads();
    // the distinct ECs of the piece: counted, then (EMIT) given consecutive places in the column's stretch of the output
    u32 mine = 0;
    for (u32 q = threadIdx.x; q < tsz; q += CVU_TPB) mine += tkey[q] != 0xFFFFFFFFu ? 1u : 0u;
    const u32 at = mine ? atomicAdd(&s_n, mine) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_n) { if (EMIT) s_base = colbase[l] + atomicAdd(&colcur[l], s_n); else atomicAdd(&colcnt[l], s_n); }
    if (!EMIT) return;
    __syncthreads();
    u32 rnk = at;
    for (u32 q = threadIdx.x; q < tsz; q += CVU_TPB) {
        const u32 e = tkey[q];
        if (e == 0xFFFFFFFFu) continue;
        const u64 pos = (u64)s_base + rnk++;
        if (pos < nnz) { keys[pos] = ((u64)e << 32) | l; vals[pos] = tmask[q]; }
    }
}
// sorted (row << 32 | column, value) pairs -> a CSR's (or CSC's) indices, data and pointers: the column is the low half of the key,
// row r starts at the first key of row r or above
__global__ void k_split_out(const u64* keys, const u32* vals, u64 nnz, int* indices, int* data) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < nnz) { indices[i] = (int)(u32)keys[i]; data[i] = (int)vals[i]; }
}
__global__ void k_row_ptr(const u64* keys, u64 nnz, u32 n_rows, int* indptr) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r <= n_rows) indptr[r] = (int)lower_bound_u64(keys, nnz, r << 32);
}
__global__ void k_cv_back_expand(const int* cscptr, const int* cscidx, u64 total, u32 n_loci, u32 n_haps, const u64* hap_start,
                                 u64* keys, u32* vals) {
    const u64 g = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (g >= total) return;
    u32 h = 0;
    while (h + 1 < n_haps && hap_start[h + 1] <= g) ++h;
    const int* ptr = cscptr + (u64)h * (n_loci + 1);
    const u64 j = g - hap_start[h];
    u32 lo = 0, hi = n_loci;                                 // column of entry j: last t with ptr[t] <= j
    while (lo < hi) { const u32 m = (lo + hi + 1) >> 1; if ((u64)ptr[m] <= j) lo = m; else hi = m - 1; }
    keys[g] = (u64)(u32)cscidx[g] * n_loci + lo;
    vals[g] = 1u << h;
}
__global__ void k_cv_back_emit(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 total, u32 n_loci,
                               int* indices, int* data) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= total || !flag[i]) return;
    u32 m = 0;
    for (u64 j = i; j < total && keys[j] == keys[i]; ++j) m |= vals[j];
    indices[pos[i]] = (int)(keys[i] % n_loci);
    data[pos[i]] = (int)m;
}
__global__ void k_cv_back_rowptr(const u64* keys, const u32* pos, u64 total, u32 nnz, u32 n_ecs, u32 n_loci, int* indptr) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e > n_ecs) return;
    const u64 at = lower_bound_u64(keys, total, (u64)e * n_loci);
    indptr[e] = at < total ? (int)pos[at] : (int)nnz;       // pos[] = index of the run that starts at or after `at`
}

// ---- CSR(bitmask) -> per-haplotype CSC as a transposition of the NON-ZEROS (bin_utils.py:979-995, Sparse3DMatrix.py:189-193) ----
// The non-zeros (locus, EC, mask) are sorted by locus -- stable, so ECs stay ascending within a column -- which is the whole
// transposition: 12 M elements and the digits of the locus alone (three 8-bit passes at 80 k loci), not the 79 M set bits and the
// digits of (haplotype, locus).  A haplotype's row indices are then the ECs of the sorted non-zeros that carry its bit, in
// that order: one counting pass per block of CVB non-zeros, one scan over (haplotype, block), one pass that writes.
constexpr int CVB = 1024;
__global__ __launch_bounds__(TPB) void k_cv_bits(const int* data, u64 nnz, u64* total) {
    u64 v = 0;
    for (u64 i = blockIdx.x * (u64)TPB + threadIdx.x; i < nnz; i += (u64)gridDim.x * TPB) v += __popc((u32)data[i]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(total, v);
}
// one thread per row: key = locus << 32 | EC, value = mask; what a .bin of unknown origin may hold is checked here
__global__ void k_cv_keys(const int* indptr, u32 n_ecs, const int* indices, const int* data, u64 nnz, u32 n_loci, u32 n_haps,
                          u64* keys, u32* vals, u32* err) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n_ecs) return;
    const long long a = indptr[e], b = indptr[e + 1];
    if (a < 0 || b < a || (u64)b > nnz || (e == 0 && a != 0)) { atomicOr(err, 1u); return; }
    bool bad = false;
    for (long long i = a; i < b; ++i) {
        const u32 lc = (u32)indices[i], m = (u32)data[i];
        bad |= lc >= n_loci || m == 0u || (m >> n_haps) != 0u;
        keys[i] = ((u64)lc << 32) | (u32)e;
        vals[i] = m;
    }
    if (bad) atomicOr(err, 2u);
}
__global__ __launch_bounds__(TPB) void k_cv_cnt(const u32* masks, u64 nnz, u32 n_haps, u32 nb, u32* blk) {
    __shared__ u32 cnt[32];
    if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
    __syncthreads();
    const u64 i0 = (u64)blockIdx.x * CVB;
#pragma unroll
    for (int r = 0; r < CVB / TPB; ++r) {
        const u64 i = i0 + (u64)r * TPB + threadIdx.x;
        const u32 m = i < nnz ? masks[i] : 0u;
        for (u32 h = 0; h < n_haps; ++h) {
            const u64 bm = __ballot((m >> h) & 1u);
            if ((threadIdx.x & 63u) == 0 && bm) atomicAdd(&cnt[h], (u32)__popcll(bm));
        }
    }
    __syncthreads();
    if (threadIdx.x < n_haps) blk[(u64)threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];
}
// scan[h * nb + b]: set bits of haplotype h before block b, counted on from the haplotypes before it -- the place of the block's
// first such bit in the row-index array.  headval[h * n_loci + t]: where column t of haplotype h starts within h's own block.
// VAL: a payload goes along -- base[i]: where the values of sorted non-zero i start in `values` (bit order: its set bits lowest first);
// the value of bit h lands in cscdata where its row index lands in cscidx
template <bool VAL>
__global__ __launch_bounds__(TPB) void k_cv_emit(const u64* keys, const u32* masks, u64 nnz, u32 n_haps, u32 n_loci, u32 nb,
                                                 const u32* scan, int* cscidx, u32* headval, const u32* base, const double* values,
                                                 double* cscdata) {
    __shared__ u32 run[32], wcnt[TPB / 64][32];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (tid < 32) run[tid] = tid < n_haps ? scan[(u64)tid * nb + blockIdx.x] : 0u;
    const u64 lt = (1ull << lane) - 1ull;
    const u64 i0 = (u64)blockIdx.x * CVB;
    for (int r = 0; r < CVB / TPB; ++r) {
        const u64 i = i0 + (u64)r * TPB + tid;
        const bool have = i < nnz;
        const u64 key = have ? keys[i] : 0ull;
        const u32 m = have ? masks[i] : 0u;
        const u32 lc = (u32)(key >> 32);
        const bool head = have && (i == 0 || (u32)(keys[i - 1] >> 32) != lc);
        for (u32 h = 0; h < n_haps; ++h) {
            const u64 bm = __ballot((m >> h) & 1u);
            if (lane == 0) wcnt[w][h] = (u32)__popcll(bm);
        }
        __syncthreads();
        for (u32 h = 0; h < n_haps; ++h) {
            const u64 bm = __ballot((m >> h) & 1u);
            u32 at = run[h] + (u32)__popcll(bm & lt);
            for (u32 k = 0; k < w; ++k) at += wcnt[k][h];
            if ((m >> h) & 1u) {
                cscidx[at] = (int)(u32)key;
                if (VAL) cscdata[at] = values[base[i] + (u32)__popc(m & ((1u << h) - 1u))];
            }
            if (head) headval[(u64)h * n_loci + lc] = at - scan[(u64)h * nb];
        }
        __syncthreads();
        if (tid < n_haps) { u32 c = 0; for (u32 k = 0; k < TPB / 64; ++k) c += wcnt[k][tid]; run[tid] += c; }
        __syncthreads();
    }
}
// column pointers: column t of haplotype h starts where the first non-empty column at or after t does
__global__ void k_cv_ptr(const u64* keys, u64 nnz, u32 n_loci, u32 n_haps, u32 nb, const u32* scan, const u64* grand, const u32* headval, int* cscptr) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t > n_loci) return;
    const u64 at = lower_bound_u64(keys, nnz, t << 32);
    const u32 t2 = at < nnz ? (u32)(keys[at] >> 32) : 0u;
    for (u32 h = 0; h < n_haps; ++h) {
        const u32 tot = (h + 1 < n_haps ? scan[(u64)(h + 1) * nb] : (u32)*grand) - scan[(u64)h * nb];
        cscptr[(u64)h * (n_loci + 1) + t] = (int)(at < nnz ? headval[(u64)h * n_loci + t2] : tot);
    }
}

// the payload's twin of the sort's value: sorted non-zero p is non-zero idx[p] of the CSR -- its mask, and where its values start
__global__ __launch_bounds__(TPB) void k_cvv_bits(const int* data, u64 nnz, u32* bits) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < nnz) bits[i] = (u32)__popc((u32)data[i]);
}
__global__ __launch_bounds__(TPB) void k_cvv_gather(const u32* idx, const int* data, const u32* bits_excl, u64 nnz, u32* masks, u32* base) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x;
    if (p >= nnz) return;
    const u32 i = idx[p];
    masks[p] = (u32)data[i];
    base[p] = bits_excl[i];
}

__global__ void k_iota(u32* out, u64 n) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) out[i] = (u32)i;
}
__global__ void k_read_ec(const u32* read_slot, u64 n, const u32* rank_of_slot, int* out) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) out[i] = read_slot[i] == 0xFFFFFFFFu ? -1 : (int)rank_of_slot[read_slot[i]];
}
__global__ void k_range_len(const int2* rng, u64 n, long long* out) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) { const int2 r = rng[i]; out[i] = r.y == INT_MIN ? 0ll : (long long)r.y - (long long)r.x + 1ll; }
}
__global__ void k_fill_minmax(int2* p, u64 n) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) p[i] = make_int2(INT_MAX, INT_MIN);
}
__global__ void k_split_minmax(const int2* rng, u64 n, int* mn, int* mx) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) { const int2 r = rng[i]; mn[i] = r.x; mx[i] = r.y; }
}
// the used stretches of the key arena, back to zero (ecb_reset): blockIdx.y = stretch
struct ArenaClear { u64 start[ARENA_REGIONS + 1], len[ARENA_REGIONS + 1]; };
__global__ void k_clear_arena(uint2* arena, ArenaClear A) {
    const u64 s = A.start[blockIdx.y], n = A.len[blockIdx.y];
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) arena[s + i] = make_uint2(0u, 0u);
}
__global__ void k_clear_slots(Slot* table, const u32* list, u64 n) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4* s = reinterpret_cast<uint4*>(table + list[i]);
    const uint4 z = make_uint4(0, 0, 0, 0);
    s[0] = z; s[1] = z; s[2] = z; s[3] = z;
}

// ---------------------------------------------------------------------------------------------
// LSD radix sort of (u64 key, u32 value) pairs, 8 bits per pass, stable: the sort behind the multisample triples
// (bam_utils_multisample.py:503-576, 737-791) and the sparse-format conversions (bin_utils.py:979-1028).
// A pass = k_rs_hist (LDS histogram per 4 096-key tile) -> exclusive scan over (digit, tile) -> k_rs_scatter.  The scatter
// ranks keys WITHOUT reordering equal digits: every wave owns a contiguous quarter of the tile and walks it 64 keys at a
// time; lanes with the same digit find each other with eight ballots (one per digit bit), the lowest of them bumps the
// wave's LDS counter of that digit by the group's size, and a key's rank is that counter value plus the number of group
// members in lower lanes.  Counters of the four waves are added up in wave order afterwards.
// ---------------------------------------------------------------------------------------------
#ifndef ECB_RS_TPB
#define ECB_RS_TPB 1024
#endif
constexpr int RS_TPB = ECB_RS_TPB, RS_TILE = 4096, RS_ITEMS = RS_TILE / RS_TPB;
static_assert(RS_TPB >= 256 && RS_TPB % 64 == 0 && RS_TILE % RS_TPB == 0, "one thread per digit among the first 256");
constexpr int RS_MAX_PASSES = 8;
// Round 3: a pass is ONE kernel.  The digit histograms of all passes are taken in one sweep up front (they do not depend on the
// order of the keys), which gives every pass the first place of each digit; where a TILE's keys of a digit go within that is
// found while the pass runs, by decoupled look-back: a workgroup takes the next tile (a counter: tiles start in order), publishes
// its per-digit counts (AGG | count), walks back over the tiles before it adding up their counts until it meets one whose inclusive
// prefix is known (PFX | prefix), and publishes its own.  One 4-byte word per (tile, digit) carries status and value, written and
// read with relaxed agent-scope atomics (write-through / L2-bypassing on gfx950: one granule, nothing else to order).  A tile only
// ever waits for tiles that were started before it, so the walk ends; the polls are bounded all the same.
// (Before: a histogram kernel, three scan kernels over (digit, workgroup) counters and the scatter per pass -- a third of a pass.)
constexpr u32 RS_AGG = 1u << 30, RS_PFX = 2u << 30, RS_VAL = (1u << 30) - 1u;
constexpr u32 RS_SPIN_MAX = 1u << 24;
#ifndef ECB_RS_LOOK
#define ECB_RS_LOOK 4
#endif
constexpr int RS_LOOK = ECB_RS_LOOK;          // tiles looked back at per round trip
struct RsShifts { u32 s[RS_MAX_PASSES]; u32 n; };
__global__ __launch_bounds__(RS_TPB) void k_rs_hist_all(const u64* keys, u64 n, RsShifts sh, u32* ghist) {
    __shared__ u32 h[RS_MAX_PASSES][256];
    for (u32 q = threadIdx.x; q < RS_MAX_PASSES * 256; q += RS_TPB) (&h[0][0])[q] = 0;
    __syncthreads();
    for (u64 i = blockIdx.x * (u64)RS_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * RS_TPB) {
        const u64 k = keys[i];
        for (u32 p = 0; p < sh.n; ++p) atomicAdd(&h[p][(u32)(k >> sh.s[p]) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256u) for (u32 p = 0; p < sh.n; ++p) { const u32 c = h[p][threadIdx.x]; if (c) atomicAdd(&ghist[p * 256 + threadIdx.x], c); }
}
__global__ __launch_bounds__(256) void k_rs_bases(const u32* ghist, u32 n_passes, u32* base) {      // exclusive scan of every pass's 256 counts
    __shared__ u32 s_w[4];
    for (u32 p = 0; p < n_passes; ++p) {
        const u32 v = ghist[p * 256 + threadIdx.x];
        const u32 incl = wave_incl_scan(v);
        if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        u32 before = 0;
        for (u32 k = 0; k < (threadIdx.x >> 6); ++k) before += s_w[k];
        base[p * 256 + threadIdx.x] = before + incl - v;
        __syncthreads();
    }
}
__global__ __launch_bounds__(RS_TPB) void k_rs_pass(const u64* kin, const u32* vin, u64 n, u32 shift, const u32* base, u32* desc,
                                                    u32* ticket, u32* err, u64* kout, u32* vout) {
    // A tile is laid out digit by digit in LDS first and leaves from there: consecutive lanes then write consecutive
    // addresses of one digit's run (16 elements on average) instead of 64 lanes writing to 64 different runs.
    __shared__ u32 cnt[RS_TPB / 64][256];          // per wave: keys of each digit; then: keys of that digit in the waves before
    __shared__ u32 dstart[256];                    // first place of digit d within the tile
    __shared__ u32 gbase[256];                     // where the tile's first key of digit d goes
    __shared__ u32 s_wsum[RS_TPB / 64];
    __shared__ u32 s_tile;
    __shared__ u64 skey[RS_TILE];
    __shared__ u32 sval[RS_TILE];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    for (u32 q = tid; q < (RS_TPB / 64) * 256; q += RS_TPB) (&cnt[0][0])[q] = 0;
    __syncthreads();
    const u32 tile = s_tile;
    const u64 t0 = (u64)tile * RS_TILE;
    if (t0 >= n) return;
    const u64 w0 = t0 + (u64)w * (RS_TILE / (RS_TPB / 64));
    const u64 lt = (1ull << lane) - 1ull;
    u64 key[RS_ITEMS];
    u32 val[RS_ITEMS], rk[RS_ITEMS];
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const u64 i = w0 + (u64)r * 64 + lane;
        const bool have = i < n;
        key[r] = have ? kin[i] : 0ull;
        val[r] = have ? vin[i] : 0u;
        const u32 d = (u32)(key[r] >> shift) & 255u;
        u64 peers = __ballot(have);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const u32 below = (u32)__popcll(peers & lt);
        u32 bs = 0;
        if (have && below == 0u) bs = atomicAdd(&cnt[w][d], (u32)__popcll(peers));
        bs = __shfl(bs, have ? __ffsll((long long)peers) - 1 : (int)lane);
        rk[r] = bs + below;
    }
    __syncthreads();
    u32 tot = 0;                                   // digit tid: its keys in the tile, and -- in place of the per-wave counts -- the keys of the waves before
    const bool dig = tid < 256u;                   // (threads beyond the 256 digits only rank and move keys)
    const u32 dt = dig ? tid : 0u;
    if (dig) {
#pragma unroll
        for (int k = 0; k < RS_TPB / 64; ++k) { const u32 c = cnt[k][tid]; cnt[k][tid] = tot; tot += c; }
    }
    // publish the tile's count of digit tid, look back for the keys of that digit in the tiles before, publish the prefix
    u32* const mine = desc + (u64)tile * 256 + dt;
    u32 excl = 0;
    if (!dig) {
    } else if (tile == 0) {
        __hip_atomic_store(mine, RS_PFX | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __hip_atomic_store(mine, RS_AGG | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u32 spins = 0;
        bool done = false;
        for (long long t = (long long)tile - 1; t >= 0 && !done;) {
            // four tiles back per round trip (their words are independent loads); consumed in order, up to the first that has nothing yet
            u32 v[RS_LOOK];
#pragma unroll
            for (int k = 0; k < RS_LOOK; ++k)
                v[k] = t - k >= 0 ? __hip_atomic_load(desc + (u64)(t - k) * 256 + dt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            int used = 0;
#pragma unroll
            for (int k = 0; k < RS_LOOK; ++k) {
                if (done || used != k || t - k < 0) continue;
                if (v[k] < RS_AGG) continue;         // nothing published there yet: this one again in the next round
                excl += v[k] & RS_VAL;
                used = k + 1;
                if (v[k] >= RS_PFX) done = true;
            }
            t -= used;
            if (!used) {
                if (++spins > RS_SPIN_MAX) { atomicOr(err, 1u); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        __hip_atomic_store(mine, RS_PFX | ((excl + tot) & RS_VAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (dig) gbase[tid] = base[tid] + excl;
    {
        const u32 incl = wave_incl_scan(tot);
        if (lane == 63) s_wsum[w] = incl;          // (waves beyond the fourth: zeros)
        __syncthreads();
        u32 before = 0;
        for (u32 k = 0; k < w; ++k) before += s_wsum[k];
        if (dig) dstart[tid] = before + incl - tot;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const u64 i = w0 + (u64)r * 64 + lane;
        if (i < n) {
            const u32 d = (u32)(key[r] >> shift) & 255u;
            const u32 lp = dstart[d] + cnt[w][d] + rk[r];
            skey[lp] = key[r]; sval[lp] = val[r];
        }
    }
    __syncthreads();
    const u32 n_tile = (u32)min((u64)RS_TILE, n - t0);
    for (u32 i = tid; i < n_tile; i += RS_TPB) {
        const u64 k = skey[i];
        const u32 d = (u32)(k >> shift) & 255u;
        const u64 pos = (u64)gbase[d] + (i - dstart[d]);
        if (pos < n) { kout[pos] = k; vout[pos] = sval[i]; }      // (always, unless a look-back gave up: reported through *err)
    }
}
__global__ __launch_bounds__(TPB) void k_or_reduce(const u64* keys, u64 n, u64* out) {
    u64 v = 0;
    for (u64 i = blockIdx.x * (u64)TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TPB) v |= keys[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
    if ((threadIdx.x & 63u) == 0 && v) atomicOr(out, v);
}
// ---------------------------------------------------------------------------------------------
// Multisample K4' / K5' (bam_utils_multisample.py:503-636, 737-791) from the (EC, cell, file) triples: cell order = insertion
// order of the reference's cr_totals (files in order; within a file ECs by first appearance there; within an EC cells by
// first appearance), per-cell totals, minimum-count filter, EC re-rank, CSC N, rows of A that survive.
// ---------------------------------------------------------------------------------------------
// Per cell: its reads, and the first file it has reads in (the reference walks the files in order: that file decides where the
// cell enters cr_totals).  Counters and minima are kept in LDS per workgroup and flushed once (n_cells <= MSF_LDS_CELLS); more
// cells than that go to memory directly.
constexpr u32 MSF_LDS_CELLS = 8192;
constexpr int TPB_MSF = 1024;
__global__ __launch_bounds__(TPB_MSF) void k_msf2_cells(const u32* meta, const u32* cnt, u64 n, u32 n_cells, u64* total, u32* firstfile, u32* err) {
    extern __shared__ u32 sh32[];                            // lfile[n_cells] | lcnt[n_cells]
    const bool lds = n_cells <= MSF_LDS_CELLS;
    u32 *lfile = sh32, *lcnt = sh32 + (lds ? n_cells : 0);
    if (lds) {
        for (u32 c = threadIdx.x; c < n_cells; c += TPB_MSF) { lfile[c] = 0xFFFFFFFFu; lcnt[c] = 0; }
        __syncthreads();
    }
    const u64 per = (n + gridDim.x - 1) / gridDim.x, t0 = blockIdx.x * per, t1 = min(t0 + per, n);
    for (u64 t = t0 + threadIdx.x; t < t1; t += TPB_MSF) {
        const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u), f = m >> ECB_CELL_BITS;
        if (c >= n_cells) { atomicOr(err, 2u); continue; }   // (cells are the ids the host handed out, 0 .. n_cells - 1)
        if (lds) { atomicAdd(&lcnt[c], cnt[t]); atomicMin(&lfile[c], f); }
        else { atomicAdd(&total[c], (u64)cnt[t]); atomicMin(&firstfile[c], f); }
    }
    if (!lds) return;
    __syncthreads();
    for (u32 c = threadIdx.x; c < n_cells; c += TPB_MSF)
        if (lfile[c] != 0xFFFFFFFFu) { atomicAdd(&total[c], (u64)lcnt[c]); atomicMin(&firstfile[c], lfile[c]); }
}
// seg[e] = first triple of EC e (the triples are sorted by EC; an EC without triples gets an empty stretch), seg[n_ecs] = n
__global__ void k_msf2_seg(const u32* ec, u64 n, u32 n_ecs, u32* seg, u32* err) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u32 e = ec[t];
    if (e >= n_ecs) { atomicOr(err, 1u); return; }
    const long long ep = t ? (long long)ec[t - 1] : -1ll;
    for (long long x = ep + 1; x <= (long long)e; ++x) seg[x] = (u32)t;
    if (t == n - 1) for (u64 x = (u64)e + 1; x <= n_ecs; ++x) seg[x] = (u32)n;
}
// Per EC: (i) the EC's first appearance in every file it has reads in -- the smallest first read among its triples of that
// file; (ii) every triple whose file is its cell's first file offers the cell (first appearance of the EC in that file, first
// read of the triple) -- the smallest offer is where the cell enters the reference's cr_totals (bam_utils_multisample.py:
// 513-546); (iii) whether any of the EC's cells survives the minimum count.
// One THREAD per EC of up to MSF_SMALL triples (the run of the mill: two dozen triples; the few triples that make an offer look
// their file's first appearance up by walking the EC's stretch again -- neighbours' stretches follow each other in memory), one
// WORKGROUP per larger EC, queued by the first kernel, with the per-file table in LDS.  (One wave per EC with three dependent
// sweeps was latency: 14 us per EC.)
// A triple whose cell is not below n_cells is passed over by every kernel here (k_msf2_cells has reported it: the call fails once
// they are done), so that total / firstfile / cellkey -- n_cells entries each -- are never read or written past their end.
constexpr u32 MSF_SMALL = 256;
constexpr u32 MSF_FILES = 1u << MS_FILE_BITS;
constexpr u32 MSF_GIANT = 1u << 15;           // triples above which an EC is shared out over the whole grid (k_msf2_giant_*), not given to one workgroup
__global__ void k_msf2_ecs_small(const u32* meta, const u32* first, const u32* seg, u32 n_ecs, u32 n_cells, const u64* total, const u32* firstfile,
                                 u64 min_count, u64* cellkey, u32* keep_ec, u32* big, u32* n_big, u32* giant, u32* n_giant) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n_ecs) return;
    const u32 a = seg[e], b = seg[e + 1];
    if (b - a > MSF_GIANT) { giant[atomicAdd(n_giant, 1u)] = (u32)e; return; }
    if (b - a > MSF_SMALL) { big[atomicAdd(n_big, 1u)] = (u32)e; return; }
    bool keep = false;
    u32 last_f = 0xFFFFFFFFu, last_fec = 0;                                  // (the EC's first appearance in the file asked for last: cells' first files repeat)
    for (u32 t = a; t < b; ++t) {
        const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u), f = m >> ECB_CELL_BITS;
        if (c >= n_cells) continue;
        keep |= total[c] >= min_count;
        if (firstfile[c] != f) continue;
        if (f != last_f) {
            u32 fec = first[t];
            for (u32 x = a; x < b; ++x) if ((meta[x] >> ECB_CELL_BITS) == f) fec = min(fec, first[x]);
            last_f = f; last_fec = fec;
        }
        const u32 fec = last_fec;
        const u64 offer = ((u64)fec << 32) | first[t];
        if (offer < cellkey[c]) atomicMin(&cellkey[c], offer);               // (the plain read may be stale: then one atomic too many)
    }
    if (keep) keep_ec[e] = 1u;
}
__global__ __launch_bounds__(TPB) void k_msf2_ecs_big(const u32* meta, const u32* first, const u32* seg, const u32* big, const u32* n_big, u32 n_cells,
                                                      const u64* total, const u32* firstfile, u64 min_count, u64* cellkey, u32* keep_ec) {
    __shared__ u32 fec[MSF_FILES];
    __shared__ u32 s_keep;
    for (u32 q = blockIdx.x; q < *n_big; q += gridDim.x) {
        const u32 e = big[q], a = seg[e], b = seg[e + 1];
        for (u32 f = threadIdx.x; f < MSF_FILES; f += TPB) fec[f] = 0xFFFFFFFFu;
        if (threadIdx.x == 0) s_keep = 0;
        __syncthreads();
        bool keep = false;
        for (u32 t = a + threadIdx.x; t < b; t += TPB) {
            const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u);
            if (c >= n_cells) continue;
            atomicMin(&fec[m >> ECB_CELL_BITS], first[t]);
            keep |= total[c] >= min_count;
        }
        if (keep) s_keep = 1u;
        __syncthreads();
        for (u32 t = a + threadIdx.x; t < b; t += TPB) {
            const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u), f = m >> ECB_CELL_BITS;
            if (c < n_cells && firstfile[c] == f) {
                const u64 offer = ((u64)fec[f] << 32) | first[t];
                if (offer < cellkey[c]) atomicMin(&cellkey[c], offer);
            }
        }
        if (threadIdx.x == 0 && s_keep) keep_ec[e] = 1u;
        __syncthreads();
    }
}
// The few ECs with tens of thousands of triples and more (config 4's most popular EC has millions): one workgroup each was the tail of the
// whole filter.  Every workgroup of the grid takes a strided share of each such EC: first the EC's first appearance per file (LDS, then one
// global atomic per file and workgroup), then -- a launch later -- the offers.
__global__ __launch_bounds__(TPB) void k_msf2_giant_fec(const u32* meta, const u32* first, const u32* seg, const u32* giant, const u32* n_giant, u32 n_cells,
                                                        const u64* total, u64 min_count, u32* gfec, u32* keep_ec) {
    __shared__ u32 fec[MSF_FILES];
    __shared__ u32 s_keep;
    for (u32 g = 0; g < *n_giant; ++g) {
        const u32 e = giant[g], a = seg[e], b = seg[e + 1];
        for (u32 f = threadIdx.x; f < MSF_FILES; f += TPB) fec[f] = 0xFFFFFFFFu;
        if (threadIdx.x == 0) s_keep = 0;
        __syncthreads();
        bool keep = false;
        for (u64 t = (u64)a + (u64)blockIdx.x * TPB + threadIdx.x; t < b; t += (u64)gridDim.x * TPB) {
            const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u);
            if (c >= n_cells) continue;
            atomicMin(&fec[m >> ECB_CELL_BITS], first[t]);
            keep |= total[c] >= min_count;
        }
        if (keep) s_keep = 1u;
        __syncthreads();
        for (u32 f = threadIdx.x; f < MSF_FILES; f += TPB) if (fec[f] != 0xFFFFFFFFu) atomicMin(&gfec[(u64)g * MSF_FILES + f], fec[f]);
        if (threadIdx.x == 0 && s_keep) keep_ec[e] = 1u;
        __syncthreads();
    }
}
__global__ __launch_bounds__(TPB) void k_msf2_giant_offer(const u32* meta, const u32* first, const u32* seg, const u32* giant, const u32* n_giant, u32 n_cells,
                                                          const u32* firstfile, const u32* gfec, u64* cellkey) {
    for (u32 g = 0; g < *n_giant; ++g) {
        const u32 e = giant[g], a = seg[e], b = seg[e + 1];
        for (u64 t = (u64)a + (u64)blockIdx.x * TPB + threadIdx.x; t < b; t += (u64)gridDim.x * TPB) {
            const u32 m = meta[t], c = m & ((1u << ECB_CELL_BITS) - 1u), f = m >> ECB_CELL_BITS;
            if (c < n_cells && firstfile[c] == f) {
                const u64 offer = ((u64)gfec[(u64)g * MSF_FILES + f] << 32) | first[t];
                if (offer < cellkey[c]) atomicMin(&cellkey[c], offer);
            }
        }
    }
}
// cells that have reads, as the lists the ordering below works on
__global__ void k_msf2_cellflag(const u64* total, u32 n_cells, u32* flag) {
    const u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (c < n_cells) flag[c] = total[c] ? 1u : 0u;
}
__global__ void k_msf2_celllist(const u64* total, const u32* firstfile, const u64* cellkey, const u32* flag, const u32* pos, u32 n_cells,
                                u32* cell_id, u64* ctotal, u64* bhi, u64* blo) {
    const u64 c = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (c >= n_cells || !flag[c]) return;
    const u32 o = pos[c];
    cell_id[o] = (u32)c; ctotal[o] = total[c]; bhi[o] = firstfile[c]; blo[o] = cellkey[c];
}
// (EC, cell) pairs that survive: a pair = the triples of one EC and one cell, which follow each other (one per file)
__global__ void k_msf2_pairflag(const u32* ec, const u32* meta, u64 n, const u32* new_cell, u32* flag) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u32 c = meta[t] & ((1u << ECB_CELL_BITS) - 1u);
    const bool head = t == 0 || ec[t - 1] != ec[t] || (meta[t - 1] & ((1u << ECB_CELL_BITS) - 1u)) != c;
    flag[t] = (head && new_cell[c] != 0xFFFFFFFFu) ? 1u : 0u;
}
__global__ void k_msf2_pairs(const u32* ec, const u32* meta, const u32* cnt, const u32* flag, const u32* pos, u64 n, const u32* new_cell,
                             const u32* new_rank, u64* key, u32* val, u32* err) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n || !flag[t]) return;
    const u32 e = ec[t], c = meta[t] & ((1u << ECB_CELL_BITS) - 1u);
    u64 sum = 0;
    for (u64 x = t; x < n && ec[x] == e && (meta[x] & ((1u << ECB_CELL_BITS) - 1u)) == c; ++x) sum += cnt[x];   // (the same cell's reads of one EC in several files add up, :737-791)
    if (sum > 0x7FFFFFFFull) atomicOr(err, 4u);             // (an entry of N is an int32)
    key[pos[t]] = ((u64)new_cell[c] << 32) | new_rank[e];
    val[pos[t]] = (u32)sum;
}
__global__ void k_msf_gather64(const u64* src, const u32* idx, u64 n, u64* dst) { const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; if (i < n) dst[i] = src[idx[i]]; }
__global__ void k_msf_keepflag(const u32* order, const u64* total, u64 n, u64 min_count, u32* flag) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n) flag[i] = total[order[i]] >= min_count ? 1u : 0u;
}
__global__ void k_msf_newcell(const u32* order, const u32* flag, const u32* pos, const u32* cell_id, u64 n, u32* new_cell, u32* kept_cells) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < n && flag[i]) { const u32 c = cell_id[order[i]]; new_cell[c] = pos[i]; kept_cells[pos[i]] = c; }
}
__global__ void k_msf_rowlen(const u32* indptr, const u32* keep_ec, const u32* new_rank, u64 n_ecs, u32* rowlen2) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e < n_ecs && keep_ec[e]) rowlen2[new_rank[e]] = indptr[e + 1] - indptr[e];
}
__global__ void k_msf_rows(const u32* indptr, const int* indices, const int* data, const u32* keep_ec, const u32* new_rank,
                           const u32* indptr2, u64 n_ecs, int* indices2, int* data2) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= n_ecs || !keep_ec[e]) return;
    const u32 a = indptr[e], b = indptr[e + 1], o = indptr2[new_rank[e]];
    for (u32 i = a; i < b; ++i) { indices2[o + (i - a)] = indices[i]; data2[o + (i - a)] = data[i]; }
}

// ---- device memory: one owner per buffer ------------------------------------------------------------------------------------------------
// A move-only buffer: its pointer, its size in bytes and the device it was allocated on, where it is freed when it goes.  It stands in for
// a T* where one is used (kernel arguments, StreamCold, pointer arithmetic): only the ownership lives here.  Three ways to fill it:
//   alloc  -- fresh: exactly max(n, at_least) bytes;
//   regrow -- kept while it holds `need` bytes, else freed and need + slack bytes taken in its place (the contents are not kept);
//   grow   -- a new n-byte buffer, filled with the byte `fill` (-1: not filled), the first `keep` bytes of the old one copied over on `st`
//             and waited for, then the old one freed (no copy and no wait when there is none).  A failing step leaves the old one in place.
// alloc and regrow free what the buffer held before they allocate.
//
// ECB_POISON_SCRATCH (a debug switch, read where it acts; unset, empty or "0": off): every allocation is filled with POISON_BYTE before it
// is handed out -- complete when alloc returns, since later work goes to other streams -- and scratch whose contents the library no longer
// defines is filled again where it dies (the per-device pool at the end of a Call, the handle's pool in ecb_reset: DESIGN.md section 4).
// What a kernel reads without anybody having written it is then 0x01010101 per word whatever the process did before: never zero, and
// as a stray count or index below 2^25.
constexpr int POISON_BYTE = 0x01;
inline bool poison_scratch() { const char* e = getenv("ECB_POISON_SCRATCH"); return e && *e && strcmp(e, "0") != 0; }
template <class T = void>
struct DevBuf {
    void* p = nullptr;
    u64 bytes = 0;
    int dev = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), dev(o.dev) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; dev = o.dev; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return static_cast<T*>(p); }
    T* operator->() const { return static_cast<T*>(p); }
    template <class U> U* as() const { return static_cast<U*>(p); }
    hipError_t reset() {
        hipError_t e = hipSuccess;
        if (p) { hipSetDevice(dev); e = hipFree(p); }
        p = nullptr; bytes = 0;
        return e;
    }
    hipError_t alloc(u64 n, u64 at_least = 0) {
        reset();
        n = std::max(n, at_least);
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = n;
        if (n && poison_scratch()) {
            e = hipMemset(p, POISON_BYTE, n);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) { reset(); return e; }
        }
        return hipSuccess;
    }
    hipError_t regrow(u64 need, u64 slack) { return bytes >= need ? hipSuccess : alloc(need + slack); }
    hipError_t grow(u64 n, int fill, u64 keep, hipStream_t st) {
        DevBuf q;
        hipError_t e = q.alloc(n);
        if (e == hipSuccess && fill >= 0) e = hipMemsetAsync(q.p, fill, n, st);
        if (e == hipSuccess && p) {
            e = hipMemcpyAsync(q.p, p, keep, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess) return e;
        e = reset();
        *this = std::move(q);
        return e;
    }
};
// pinned host memory, freed with its owner
struct HostFree { void operator()(void* q) const { hipHostFree(q); } };
template <class T> using Pinned = std::unique_ptr<T, HostFree>;
template <class T> hipError_t pin(Pinned<T>& out) {
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, sizeof(T), hipHostMallocDefault);
    out.reset(static_cast<T*>(q));
    return e;
}

}  // namespace

// =============================================================================================
// host side
// =============================================================================================
// Where a handle's stream stands (in this order: a stage is never left for an earlier one, except by ecb_reset) ...
enum class Stage { OPEN,              // takes pushes
                   COUNTED,           // Slot::count / first_inv hold the reads pushed (k_count ran, or entries were adopted): closed to pushes
                   FINAL };           // a result is there to export
// ... and where its table's entries came from
enum class Origin { OWN,              // its own reads (and what ecb_table_merge_device added to them)
                    ADOPTED,          // adopted entries in consecutive slots (no hashing): finalize / export only
                    ASSEMBLED };      // no table: the result was put together from per-range results (ecb_assemble_ranges_device)
// whose (EC, cell, file) triples Run::tri holds
enum class Triples { NONE, OWN /* ms_reduce, of the handle's own reads */, ADOPTED /* ecb_ms_adopt_triples_device (multi-GPU) */ };
// the instantiations of k_stream that are launched, one row of STREAM_VARIANTS each
enum StreamVariant { SV_STD, SV_STD_RANGES, SV_SHORT, SV_PAR, SV_VERIFY, SV_N };

struct ecb_handle {
    ecb_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    u64 wave_arena_n = 0;             // see StreamArgs::wave_arena
    bool scatter_attr_set = false, count_attr_set = false;
    u64 resident_blocks[SV_VERIFY] = {}, rounds = 24, min_tiles = 32;     // k_stream's launch shape, per variant (queried once: plan_stream)
    bool par_stream = false;          // batches go through ks_par::k_stream: the batch before met loci that displace each other in the LDS table (sticky per handle)
    bool ctr_synced = false;          // hctr is what the device holds (no kernel that counts has been queued since the last read-back)

    u64 cap = 0, arena_cap = 0;       // slots of table, pairs of arena
    Counters hctr{};                  // last read-back
    struct PinOut { Counters c; u64 tot[8]; };
    u64 read_slot_cap = 0;
    u64 meta_cap = 0;                 // multisample: cell | file << 22 per read
    u64 queue_cap = 0;
    u64 n_ecs() const { return hctr.n_ecs; }
    u64 reads_hint = 0;               // ecb_hint_reads: the stream holds at most this many reads (0 = not said)

    // host-pointer staging (the streams behind st_rid, in its allocation)
    u32 *st_loc = nullptr, *st_hf = nullptr; int* st_pos = nullptr; u64 st_cap = 0;

    // Everything that describes the stream being built and its results, and nothing that outlives it: ecb_reset ends in run = Run{}.
    // (The pointers are views into pool buffers, which stay; a null one says that what it would show has not been made.)
    struct Run {
        Stage stage = Stage::OPEN;
        Origin origin = Origin::OWN;
        u32 prev_rid = 0xFFFFFFFFu;       // read_id of the last record pushed so far
        u64 n_reads = 0;
        u64 reads_hi = 0;                 // read_slot entries [0, reads_hi) may be set (n_reads, or more mid-batch)
        u64 records_pushed = 0;           // records of the batches so far (with n_reads: how many records a read brings)
        u64 meta_hi = 0;                  // meta entries [0, meta_hi) are set
        u64 extra_all = 0, extra_valid = 0, extra_reads = 0;   // counters merged in from other ranks
        u64 n_mismatch = 0;               // ECB_F_VERIFY: reads the exactness pass found in a wrong EC, over all pushes
        // A push, merge or adopt failed after it had begun to change the table: its return code and text (run_refused).  The table may hold ECs
        // of half a batch, slots whose key is DEAD_KEY and counters that match neither, so until ecb_reset every entry point but ecb_reset,
        // ecb_destroy, ecb_last_error and ecb_profile* answers ECB_ERR_STATE before it launches or copies anything (refused_run).
        int refused = ECB_OK;
        std::string refusal;
        std::vector<u32> c_rid, c_loc, c_hf; std::vector<int> c_pos;   // open read carried between pushes
        // the occupied slots, listed in pool[P_LIST]: current when d_list_n is set, which is where its length sits on the device
        // (null: not listed, or slot ids have changed since)
        u64* d_list_n = nullptr;
        // finalize's / assemble's result: A as CSR and the reads per EC (n_list: the slots finalize found occupied, pool[P_LIST])
        struct Csr { u32 *order = nullptr, *rank_of_slot = nullptr /* made on demand: ensure_slot_ranks */, *indptr = nullptr;
                     int *indices = nullptr, *data = nullptr, *counts = nullptr; } csr;
        u64 n_list = 0;
        ecb_sizes sizes{};
        // multisample: the distinct (EC, cell, file) triples, sorted (ocount null: the counts are the differences of ostart)
        struct Tri { u64 n = 0; u64* okey = nullptr; u32 *ofirst = nullptr, *ostart = nullptr, *ocount = nullptr; } tri;
        Triples triples = Triples::NONE;
        // ecb_ms_filter's result: kept cells in sample order, rows of A of the kept ECs, CSC N (cells null: none is current)
        struct Filtered { u32* cells = nullptr; int *ipa = nullptr, *ixa = nullptr, *daa = nullptr, *ipn = nullptr, *ixn = nullptr, *dan = nullptr; } flt;
        ecb_ms_sizes msf{};
    } run;
    // what the entry points ask of the lifecycle
    bool multisample() const { return (cfg.flags & ECB_F_MULTISAMPLE) != 0; }
    bool can_push() const { return run.stage == Stage::OPEN; }
    bool counted() const { return run.stage >= Stage::COUNTED; }
    bool has_result() const { return run.stage == Stage::FINAL; }
    bool has_ms_result() const { return has_result() && multisample(); }
    bool open_read() const { return !run.c_rid.empty(); }                          // a host push left a read open
    bool holds_nothing() const { return !n_ecs() && !run.n_reads && !open_read(); }
    bool entries_from_elsewhere() const { return run.origin != Origin::OWN; }      // (multi-GPU: its triples come by ecb_ms_adopt_triples_device)
    u32* slot_list() const { return pool[P_LIST].as<u32>(); }
    bool awaits_triples() const { return entries_from_elsewhere() && run.triples != Triples::ADOPTED; }

    // device scratch reused across calls (grown on demand: POOL)
    enum { P_RESUME, P_SUMS, P_HIST, P_OFFS, P_PAIRS, P_CNT, P_PARTS, P_WORK, P_LIST, P_BITMAP, P_WPOP, P_WPREFIX, P_ROWLEN, P_ORDER,
           P_WCOUNTS, P_RANK, P_INDPTR, P_COUNTS, P_INDICES, P_DATA, P_MS_KEYS, P_MS_KEYS2, P_MS_VALS, P_MS_VALS2, P_MS_TMP,
           P_MS_FLAG, P_MS_POS, P_MS_OKEY, P_MS_OFIRST, P_MS_OSTART, P_MS_X, P_MS_OCOUNT, P_MS_GRANK, P_MS_CIN, P_MS_FIN, P_LISTFN,
           P_REMAP, P_TOTALS, P_SLOW_LEN, P_SLOW_OFF, P_SLOW_NRE, P_SLOW_REQ, P_SLOW_REQ2, P_QCOMPACT, P_SLOW_KEY, P_SLOW_MASK, P_BIG, P_RS_HIST, P_RS_OFFS,
           P_F_CELLS, P_F_IPA, P_F_IXA, P_F_DAA, P_F_IPN, P_F_IXN, P_F_DAN, P_EXPORT, P_N };

    // profiling
    bool prof = false; double prof_ms = 0; u64 prof_launches = 0, prof_records = 0;
    int last_variant = SV_N;          // which variant of the stream kernel the last batch launched (ecb_profile_kernel; SV_N: no batch yet)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // The memory the handle owns, freed when it is deleted, after the stream (members go last to first: the table first, the staging last)
    DevBuf<u32> st_rid;                        // one allocation for all host-pointer staging streams (ensure_staging)
    DevBuf<> pool[P_N];
    DevBuf<StreamCold> d_cold;                 // k_stream's rarely used arguments (device copy; pin_cold is its pinned staging)
    Pinned<StreamCold> pin_cold;
    Pinned<PinOut> pin_out;                    // where the device's counters and finalize's totals land (a copy into pageable memory is staged by the runtime, behind a wait of its own)
    Pinned<Counters> pin_ctr;                  // pinned staging for clear_counters
    DevBuf<u64> wave_arena;                    // two words per wave, wave_arena_n waves
    DevBuf<u64> queue;                         // deferred reads (queue_cap of them)
    DevBuf<int2> rng;                          // ECB_F_RANGES: {min, max} of reference_start per (locus, haplotype)
    DevBuf<u32> meta;                          // meta_cap entries
    DevBuf<u32> read_slot;                     // read_slot_cap entries
    DevBuf<Counters> ctr;
    DevBuf<uint2> arena;
    DevBuf<Slot> table;

    ~ecb_handle() {
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (stream) hipStreamDestroy(stream);
    }
};

namespace {

thread_local std::string t_err;       // the text of a failing call without a handle: one per thread (ecb_last_error(NULL))

int fail(ecb_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (h) h->err = buf; else t_err = buf;
    return code;
}
// A building pass (a batch of a push, a merge, an adopt) hands its return code through here once it has begun to change the table: the
// first one that is not ECB_OK leaves the run refused (ecb_handle::Run::refused) ...
int run_refused(ecb_handle* h, int rc) {
    if (rc != ECB_OK && h->run.refused == ECB_OK) { h->run.refused = rc; h->run.refusal = h->err; }
    return rc;
}
// ... and this is what every later call on the handle answers first, until ecb_reset
int refused_run(ecb_handle* h) {
    if (h->run.refused == ECB_OK) return ECB_OK;
    return fail(h, ECB_ERR_STATE, "this run was refused (%d: %s): ecb_reset the handle", h->run.refused, h->run.refusal.c_str());
}
// a failing HIP call ends the function: "<prefix><the call>: <what HIP says>"
#define HIPCHK_AS(h, prefix, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return fail(h, ECB_ERR_HIP, "%s%s: %s", prefix, #call, hipGetErrorString(e_)); } while (0)
#define HIPCHK(h, call) HIPCHK_AS(h, "", call)
// ... and so does a call of the library's own that does not return ECB_OK (it has set the text)
#define RCCHK(call) do { const int rc_ = (call); if (rc_ != ECB_OK) return rc_; } while (0)

// Error bits a kernel leaves behind, as data: the first entry of `table` with a bit in `bits` is the refusal (ECB_OK when none is
// set), so the table's order says which one wins.  `arg` fills the one %llu a text may hold.
struct ErrBit { u32 bit; int code; const char* text; };
template <size_t N> int refuse_bits(ecb_handle* h, const ErrBit (&table)[N], u32 bits, unsigned long long arg = 0) {
    for (const ErrBit& e : table) if (bits & e.bit) return fail(h, e.code, e.text, arg);
    return ECB_OK;
}
const ErrBit COUNTER_ERRS[] = {
    {ERR_CONTRACT, ECB_ERR_CONTRACT, "read_id run counter violates the tuple contract (see ecb.h)"},
    {ERR_RANGE, ECB_ERR_CONTRACT, "locus or haplotype index out of range in a valid record"},
    {ERR_ARENA, ECB_ERR_TABLE_FULL, "EC key arena exhausted (%llu pairs): raise arena_capacity"},
    {ERR_QUEUE, ECB_ERR_TABLE_FULL, "deferred-read queue exhausted"},
    {ERR_INTERNAL, ECB_ERR_HIP, "internal: an EC-table slot was claimed but its key never published"},
    {ERR_COUNT, ECB_ERR_LIMIT, "an EC's count is above 2^31-1"},
};

u64 next_pow2(u64 x) { u64 p = 1; while (p < x) p <<= 1; return p; }
// all ones up to the highest set bit of x (0 for 0): the bits a sort of keys no larger than x has to look at
u64 msb_mask(u64 x) { return x ? ~0ull >> __builtin_clzll(x) : 0ull; }
inline unsigned nblk(u64 n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// ptr = the handle's scratch buffer `id`, holding at least max(count, 1) of what ptr points to (regrown with a quarter more)
#define POOL(h, id, ptr, count) do { const u64 need_ = std::max<u64>(count, 1) * sizeof(*(ptr)); \
    HIPCHK(h, h->pool[ecb_handle::id].regrow(need_, need_ / 4)); \
    (ptr) = h->pool[ecb_handle::id].as<std::remove_reference_t<decltype(*(ptr))>>(); } while (0)
// one call's scratch: a fresh buffer of max(n, 1) T's that lives as long as `keep` (nullptr when it cannot be had: see missing)
template <class T> T* fresh(std::vector<DevBuf<>>& keep, u64 n) {
    keep.emplace_back();
    return keep.back().alloc(std::max<u64>(n, 1) * sizeof(T)) == hipSuccess ? keep.back().as<T>() : nullptr;
}
bool missing(const std::vector<DevBuf<>>& keep) { return std::any_of(keep.begin(), keep.end(), [](const DevBuf<>& b) { return !b.p; }); }

// zero the device counters and point every arena region's cursor at its first pair
int clear_counters(ecb_handle* h) {
    Counters c{};
    const u32 R = arena_regions(h->arena_cap);
    const u64 per = h->arena_cap / R;
    for (u32 r = 0; r < ARENA_REGIONS; ++r) c.arena_reg[r] = r < R ? r * per : h->arena_cap;
    h->hctr = c;
    if (h->pin_ctr) {                               // pinned staging: queued behind the stream's work, no wait (rewritten only by the next reset,
        *h->pin_ctr = c;                            //  which comes after the waits of a push and a finalize)
        HIPCHK(h, hipMemcpyAsync(h->ctr, h->pin_ctr.get(), sizeof(Counters), hipMemcpyHostToDevice, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->ctr, &h->hctr, sizeof(Counters), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->ctr_synced = true;
    return ECB_OK;
}
// pairs of the key arena handed out so far (an upper bound of the pairs in use: the tail of a wave's last chunk is idle)
u64 arena_used(const ecb_handle* h) {
    const u32 R = arena_regions(h->arena_cap);
    const u64 per = h->arena_cap / R;
    u64 used = h->hctr.arena_top;
    for (u32 r = 0; r < R; ++r) used += std::min<u64>(h->hctr.arena_reg[r], (u64)(r + 1) * per) - r * per;
    return used;
}

int sync_counters(ecb_handle* h) {
    HIPCHK(h, hipMemcpyAsync(&h->pin_out->c, h->ctr, sizeof(Counters), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->hctr = h->pin_out->c;
    h->ctr_synced = true;
    return refuse_bits(h, COUNTER_ERRS, h->hctr.err, h->arena_cap);
}

int grow_table(ecb_handle* h, u64 new_cap) {
    DevBuf<Slot> nt;
    u32* remap = nullptr;
    if (new_cap > (1ull << 32)) return fail(h, ECB_ERR_LIMIT, "EC table beyond 2^32 slots");
    POOL(h, P_REMAP, remap, h->cap);
    HIPCHK(h, nt.alloc(new_cap * sizeof(Slot)));
    HIPCHK_AS(h, "grow_table: ", hipMemsetAsync(nt, 0, new_cap * sizeof(Slot), h->stream));
    // (slots the old table did not hold map to PENDING: read_slot may hold slot ids of an EARLIER stream beyond the reads processed so far --
    //  ecb_reset leaves them, ecb_hint_reads makes reads_hi run ahead of the stream -- and what such an entry maps to must not be pool garbage)
    HIPCHK_AS(h, "grow_table: ", hipMemsetAsync(remap, 0xFF, h->cap * sizeof(u32), h->stream));
    k_rehash<<<2048, TPB, 0, h->stream>>>(h->table, h->cap, nt, new_cap - 1, remap);
    if (h->run.reads_hi)
        k_remap_read_slot<<<2048, TPB, 0, h->stream>>>(h->read_slot, h->run.reads_hi, remap);
    HIPCHK_AS(h, "grow_table: ", hipStreamSynchronize(h->stream));
    HIPCHK(h, h->table.reset());
    h->table = std::move(nt);
    h->cap = new_cap; h->run.d_list_n = nullptr;   // (slot ids changed)
    return ECB_OK;
}

int ensure_read_slot(ecb_handle* h, u64 need) {
    if (need <= h->read_slot_cap) return ECB_OK;
    u64 nc = std::max<u64>(need, h->read_slot_cap * 2);
    nc = std::max<u64>(nc, 1024);
    HIPCHK(h, h->read_slot.grow(nc * sizeof(u32), 0xFF, h->run.n_reads * sizeof(u32), h->stream));
    h->read_slot_cap = nc;
    return ECB_OK;
}

// multisample: room in meta for reads [0, need), what is set so far kept
int ensure_meta(ecb_handle* h, u64 need) {
    if (need <= h->meta_cap) return ECB_OK;
    const u64 nc = std::max<u64>(need, h->meta_cap * 2);
    HIPCHK(h, h->meta.grow(nc * sizeof(u32), -1, h->run.meta_hi * sizeof(u32), h->stream));
    h->meta_cap = nc;
    return ECB_OK;
}

// deferred reads: measure, scratch, k_slow; grow the table and repeat while reads bounce.  All scratch lives in the
// handle's pool (a stream of long reads pays no hipMalloc per round, and no early return can leak it).
// verify: the exactness pass over the same reads (compare with the EC each was given; no insert, one round).
int run_slow(ecb_handle* h, const u32* d_rid, const u32* d_loc, const u32* d_hf, u64 n, u64* d_q, u64 nq, bool verify = false, u32 tw = 512u) {
    int rc = ECB_OK;
    int flip = 0;
    while (nq) {
        u64 *d_len = nullptr, *d_off = nullptr, *d_nre = nullptr, *nre_buf = nullptr;
        POOL(h, P_SLOW_LEN, d_len, nq); POOL(h, P_SLOW_OFF, d_off, nq); POOL(h, P_SLOW_NRE, d_nre, 1);
        if (flip) POOL(h, P_SLOW_REQ2, nre_buf, nq); else POOL(h, P_SLOW_REQ, nre_buf, nq);      // (d_q may be the other one)
        HIPCHK(h, hipMemsetAsync(d_nre, 0, sizeof(u64), h->stream));
        k_slow_len<<<(unsigned)nq, TPB, 0, h->stream>>>(d_rid, n, d_q, nq, d_len, tw);
        std::vector<u64> len(nq), off(nq);
        HIPCHK(h, hipMemcpyAsync(len.data(), d_len, nq * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        u64 tot = 0;
        for (u64 i = 0; i < nq; ++i) { off[i] = tot; tot += 2 * len[i]; }
        u32 *sk = nullptr, *sm = nullptr;
        const DevBuf<>& bk = h->pool[ecb_handle::P_SLOW_KEY];
        const DevBuf<>& bm = h->pool[ecb_handle::P_SLOW_MASK];
        const u64 had_k = bk.bytes, had_m = bm.bytes;
        POOL(h, P_SLOW_KEY, sk, tot); POOL(h, P_SLOW_MASK, sm, tot);
        // k_slow leaves its scratch zeroed: only a fresh (re)allocation needs clearing
        if (bk.bytes != had_k) HIPCHK(h, hipMemsetAsync(sk, 0, bk.bytes, h->stream));
        if (bm.bytes != had_m) HIPCHK(h, hipMemsetAsync(sm, 0, bm.bytes, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_off, off.data(), nq * sizeof(u64), hipMemcpyHostToDevice, h->stream));
        SlowArgs a{d_rid, d_loc, d_hf, d_q, d_len, d_off, sk, sm, h->cfg.n_loci, h->cfg.n_haplotypes,
                   h->table, h->cap - 1, h->arena, h->arena_cap, h->ctr, h->read_slot, h->run.reads_hi, nre_buf, d_nre, verify ? 1u : 0u};
        k_slow<<<(unsigned)nq, TPB, 2 * SLOW_LDS * sizeof(u32), h->stream>>>(a);
        u64 nre = 0;
        HIPCHK(h, hipMemcpyAsync(&nre, d_nre, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        rc = sync_counters(h);                          // (waits: `off` lives on this stack frame)
        if (rc != ECB_OK || verify) break;
        d_q = nre_buf; nq = nre; flip ^= 1;
        if (nq) { rc = grow_table(h, h->cap * 4); if (rc != ECB_OK) break; }
    }
    return rc;
}

int excl_scan(ecb_handle* h, const u32* in, u64 n, u32* out, u64* total);

// The launched instantiations of k_stream (k_stream.inc, compiled three times): the kernel, the name rocprofv3 gives it (ecb_profile_kernel;
// the exactness pass is not reported) and the workgroups per CU assumed when the occupancy query fails.
struct StreamVariantRow { void (*kernel)(StreamArgs); const char* name; int blocks_per_cu; };
const StreamVariantRow STREAM_VARIANTS[SV_N] = {
    {ks_std::k_stream<false>, "ks_std::k_stream<false, false>", 4},
    {ks_std::k_stream<false, true>, "ks_std::k_stream<false, true>", 4},      // with the range update fused in: fewer waves resident
    {ks_short::k_stream<false>, "ks_short::k_stream<false, false>", 4},       // short reads: 9.9 KB of LDS per wave, four workgroups per CU
    {ks_par::k_stream<false>, "ks_par::k_stream<false, false>", 5},
    {ks_std::k_stream<true>, "", 0},                                          // SV_VERIFY: planned with SV_STD's residency
};

// Launch shape of k_stream over n records: the stream is cut into ECB_ROUNDS x as many slices as waves are resident at
// once; the launch holds the resident waves only, which claim slice after slice.
struct StreamPlan { u64 slices, chunk, blocks, pwaves; };
int plan_stream(ecb_handle* h, u64 n, StreamPlan* P, StreamVariant v) {
    if (!h->resident_blocks[SV_STD]) {                 // (asked once per handle: two runtime queries per batch add up on a streamed BAM)
        int cus = 256;
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
        for (int i = 0; i < SV_VERIFY; ++i) {
            int bpc = STREAM_VARIANTS[i].blocks_per_cu;
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, STREAM_VARIANTS[i].kernel, TPB, 0);
            h->resident_blocks[i] = (u64)std::max(cus, 1) * std::max(bpc, 1);
        }
        h->rounds = getenv("ECB_ROUNDS") ? std::max(1, atoi(getenv("ECB_ROUNDS"))) : 24;   // (16 .. 32 measure alike on C3; fewer slices = fewer slice tails read twice)
        h->min_tiles = getenv("ECB_MIN_TILES") ? std::max(2, atoi(getenv("ECB_MIN_TILES"))) : 32;
    }
    // (k_stream<true> is not asked: the exactness pass keeps the hot kernel's shape)
    const u64 rounds = h->rounds, resident_blocks = h->resident_blocks[v == SV_VERIFY ? SV_STD : v];
    // slices: `rounds` per resident wave for balance, but not shorter than MIN_TILES tiles while every resident wave still gets
    // one -- a wave runs on past its slice's end to finish its open read, so every slice costs about one tile read twice
    // (at 5 tiles per slice, an eighth of config 3 on one of 8 GPUs, that was a fifth of the kernel)
    const u64 MIN_TILES = h->min_tiles;
    const u64 res_waves = resident_blocks * NWAVE;
    u64 waves = std::min<u64>(res_waves * rounds, std::max<u64>(n / (MIN_TILES * WT), res_waves));
    waves = std::min<u64>(waves, (n + 2 * WT - 1) / (2 * WT));
    waves = std::max<u64>(waves, 1);
    u64 chunk = (n + waves - 1) / waves;
    chunk = (chunk + WT - 1) / WT * WT;          // whole tiles: a tile never straddles two slices
    waves = (n + chunk - 1) / chunk;
    P->slices = waves; P->chunk = chunk;
    P->blocks = std::min<u64>((waves + NWAVE - 1) / NWAVE, resident_blocks);
    P->pwaves = P->blocks * NWAVE;               // waves of the launch
    // deferred reads: a parked launch defers at most the reads of the tiles in flight (one tile per resident wave); a read
    // with more than CMAX loci takes more than CMAX records
    const u64 need_q = P->pwaves * (u64)(WT + 1) + n / 64 + 16;      // (64: the smaller of the two kernels' carry limits, k_stream.inc)
    if (h->queue_cap < need_q) {
        h->queue_cap = 0;
        HIPCHK(h, h->queue.alloc(need_q * sizeof(u64)));
        h->queue_cap = need_q;
    }
    return ECB_OK;
}

// the reads a k_stream launch deferred (h->hctr.n_queue of them, in the stripes of h->queue), closed up and handed to k_slow
int run_deferred(ecb_handle* h, const u32* d_rid, const u32* d_loc, const u32* d_hf, u64 n, bool verify, u32 tw, u64* n_done = nullptr) {
    const u64 nq = h->hctr.n_queue;
    if (n_done) *n_done = nq;
    if (!nq) return ECB_OK;
    u64* d_q = nullptr;
    POOL(h, P_QCOMPACT, d_q, nq);
    k_queue_compact<<<QSTRIPES, TPB, 0, h->stream>>>(h->queue, h->queue_cap, h->ctr, d_q);
    HIPCHK(h, hipGetLastError());
    return run_slow(h, d_rid, d_loc, d_hf, n, d_q, nq, verify, tw);
}

// Which variant a batch of n records takes: ranges first, then short reads, then par.
StreamVariant pick_variant(const ecb_handle* h, u64 n) {
    if (h->rng) return SV_STD_RANGES;
    // Short reads (a 512-record tile holds more reads than a pass of 64 takes): the kernel with passes of 128 reads.  Known only when the
    // caller has said how many reads the stream holds (ecb_hint_reads) -- the records-per-read of this batch is then n / (its share of them).
    // (records per read: of the batches before this one where there are any; a first batch is judged as if it were the whole stream -- it must
    //  then hold at least one record per announced read -- so that a long-read stream pushed in many batches is not taken for a short-read one)
    const bool few = h->run.n_reads ? h->run.records_pushed < 7 * h->run.n_reads : (n >= h->reads_hint && n < 7 * h->reads_hint);
    if (h->reads_hint != 0 && h->cfg.n_loci < MAX_LOCI_SHORT && h->cfg.n_haplotypes <= 8 && !getenv("ECB_NO_SHORT") &&
        (getenv("ECB_FORCE_SHORT") || few)) return SV_SHORT;
    // Loci that displace each other in the LDS table (paralogs: target ids anywhere): the compilation whose key compare settles displaced pairs
    // in registers, once a batch has shown that more than a quarter of its tiles took the probe-on path (and back below a sixteenth).
    if (!getenv("ECB_NO_PAR") && (getenv("ECB_FORCE_PAR") || h->par_stream)) return SV_PAR;
    return SV_STD;
}

// zero the words of the counters every launch of k_stream starts from: the deferred reads' total with the stripes' counters behind it, the
// park flag and the slice cursor
int zero_launch_words(ecb_handle* h) {
    HIPCHK(h, hipMemsetAsync(&h->ctr->n_queue, 0, (1 + QSTRIPES) * sizeof(u64), h->stream));
    HIPCHK(h, hipMemsetAsync(&h->ctr->full, 0, sizeof(u32), h->stream));
    HIPCHK(h, hipMemsetAsync(&h->ctr->next_slice, 0, sizeof(u64), h->stream));
    return ECB_OK;
}

// One launch of variant v of k_stream over a batch of whole reads (read ids continuing from prev_rid), with k_sum_counts queued behind it.
// The batch's first launch (launch 0) sets the batch up: resume points, wave counts, StreamCold staged through pin_cold.  A relaunch after a park
// takes up what the parked launch left and zeroes the per-launch words only.  A push lets k_init_resume zero those, reserves the wave arena and
// has its k_stream bracketed by the profiling events; the exactness pass (SV_VERIFY) inserts nothing -- no wave arena, no ranges -- and
// counts the reads that differ: its wave counts and n_mismatch are cleared.  d_last: where k_sum_counts finds the batch's last read id (or null).
int launch_stream(ecb_handle* h, StreamVariant v, const StreamPlan& P, const u32* d_rid, const u32* d_loc, const u32* d_hf, const int* d_pos, u64 n,
                  u32 prev_rid, const u32* d_last, u32 launch, u64 offered, u64* timing = nullptr) {
    const bool verify = v == SV_VERIFY;
    int2* const rng = verify ? nullptr : (int2*)h->rng;
    u64* d_resume = nullptr; u32* d_wcounts = nullptr;
    POOL(h, P_RESUME, d_resume, 2 * P.slices);
    if (!launch) k_init_resume<<<nblk(P.slices, TPB), TPB, 0, h->stream>>>(d_resume, P.slices, P.chunk, verify ? nullptr : (Counters*)h->ctr);
    POOL(h, P_WCOUNTS, d_wcounts, 3 * P.pwaves);       // (every wave of a push's launch stores its three words when it ends)
    if (launch) RCCHK(zero_launch_words(h));
    else {
        if (verify) {
            HIPCHK(h, hipMemsetAsync(d_wcounts, 0, 3 * P.pwaves * sizeof(u32), h->stream));
            RCCHK(zero_launch_words(h));
            HIPCHK(h, hipMemsetAsync(&h->ctr->n_mismatch, 0, sizeof(u64), h->stream));
        } else if (h->wave_arena_n < P.pwaves) {        // (only ever grows to the resident wave count; zero = nothing reserved)
            HIPCHK(h, h->wave_arena.grow(2 * P.pwaves * sizeof(u64), 0, 2 * h->wave_arena_n * sizeof(u64), h->stream));
            h->wave_arena_n = P.pwaves;
        }
        // (pinned: rewritten by the next batch, which starts after this one's host wait)
        *h->pin_cold = StreamCold{h->arena, h->arena_cap, h->queue, h->queue_cap, d_resume, d_wcounts, verify ? nullptr : (u64*)h->wave_arena, timing,
                                  P.chunk, prev_rid, d_pos, rng, verify ? 0u : h->cfg.n_loci, verify ? 0u : h->cfg.n_haplotypes};
        HIPCHK(h, hipMemcpyAsync(h->d_cold, h->pin_cold.get(), sizeof(StreamCold), hipMemcpyHostToDevice, h->stream));
    }
    const StreamArgs a{d_rid, d_loc, d_hf, n, h->table, h->cap - 1, h->ctr, h->read_slot, h->run.reads_hi, h->d_cold,
                       !verify && getenv("ECB_ABLATE") ? (u32)atoi(getenv("ECB_ABLATE")) : 0u, d_pos, rng};
    if (h->prof && !verify) hipEventRecord(h->ev0, h->stream);
    STREAM_VARIANTS[v].kernel<<<(unsigned)P.blocks, TPB, 0, h->stream>>>(a);
    if (h->prof && !verify) hipEventRecord(h->ev1, h->stream);
    k_sum_counts<<<1, 1024, 0, h->stream>>>(d_wcounts, P.pwaves, h->ctr, verify ? 1u : 0u, offered, h->queue_cap, d_last);
    HIPCHK(h, hipGetLastError());
    if (!verify) h->last_variant = v;
    return ECB_OK;
}

// The exactness pass over one device-resident batch (whole reads, read ids continuing from prev_rid): every read's target
// set is derived again from its records and compared, pair by pair, with the key of the EC the read was given.
// Reads longer than a tile go through k_slow's compare.  *n_mismatch = reads in a wrong EC (0 = exact); *n_long = how many
// took the long path.
int verify_pass(ecb_handle* h, const StreamPlan& P, const u32* d_rid, const u32* d_loc, const u32* d_hf, u64 n, u32 prev_rid, u64* n_long, u32 tw) {
    RCCHK(launch_stream(h, SV_VERIFY, P, d_rid, d_loc, d_hf, nullptr, n, prev_rid, nullptr, 0, 0));
    RCCHK(sync_counters(h));
    return run_deferred(h, d_rid, d_loc, d_hf, n, true, tw, n_long);
}
int verify_batch(ecb_handle* h, const u32* d_rid, const u32* d_loc, const u32* d_hf, u64 n, u32 prev_rid, u64* n_mismatch, u64* n_long, u32 tw = 512u) {
    StreamPlan P;
    RCCHK(plan_stream(h, n, &P, SV_VERIFY));
    u64 nq = 0;
    if (const int rc = verify_pass(h, P, d_rid, d_loc, d_hf, n, prev_rid, &nq, tw); rc != ECB_OK) {
        // The pass built nothing, so what it refused is the stream it was shown, not the run (ecb.h): the error bits its kernels left go with the
        // refusal -- left standing, they were reported once more by whichever call read the counters next, a push or a finalize of sound input.
        // (No run with a bit of its own gets here: it is a refused run, which verify_streams and process_batch answer first.)
        if (h->hctr.err) {
            const std::string refusal = h->err;          // (a clear that fails is its own error; one that succeeds leaves the refusal's text)
            HIPCHK(h, hipMemsetAsync(&h->ctr->err, 0, sizeof(u32), h->stream));
            HIPCHK(h, hipMemsetAsync(&h->ctr->n_queue, 0, (1 + QSTRIPES) * sizeof(u64), h->stream));
            h->hctr.err = 0; h->hctr.n_queue = 0;
            h->err = refusal;
        }
        return rc;
    }
    *n_mismatch = h->hctr.n_mismatch;
    *n_long = nq;
    HIPCHK(h, hipMemsetAsync(&h->ctr->n_queue, 0, (1 + QSTRIPES) * sizeof(u64), h->stream));      // (the queue is drained: not a launch, the other per-launch words stay)
    h->hctr.n_queue = 0;
    return ECB_OK;
}

// one batch of whole reads, device-resident (*launched: the batch's kernels were queued, so a failure leaves the table half built)
int build_batch(ecb_handle* h, const u32* d_rid, const u32* d_loc, const u32* d_hf, const int* d_pos, u64 n, u32 tw, bool* launched) {
    if (n == 0) return ECB_OK;
    // How many reads the stream holds after this batch: the read id of its last record, fetched before anything is launched -- or,
    // when the caller has said how many reads the whole stream holds at most (ecb_hint_reads), that bound now and the
    // exact number with the counters, at the batch's one wait.
    const bool hinted = h->reads_hint != 0;
    u32 last_rid = 0;
    u64 reads_after = std::max<u64>(h->reads_hint, h->run.n_reads);
    if (!hinted) {
        HIPCHK(h, hipMemcpyAsync(&last_rid, d_rid + rec_at(n - 1, tw), sizeof(u32), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        reads_after = (u64)(u32)(last_rid + 1u);
        if (reads_after < h->run.n_reads) return fail(h, ECB_ERR_CONTRACT, "read_id went backwards across pushes");
    }
    RCCHK(ensure_read_slot(h, reads_after));
    h->run.reads_hi = reads_after;
    // keep the table at most half full before a batch (it grows again, via k_slow, if a batch overfills it)
    while (h->n_ecs() * 2 > h->cap) { RCCHK(grow_table(h, h->cap * 4)); }
    const StreamVariant v = pick_variant(h, n);
    StreamPlan P;
    RCCHK(plan_stream(h, n, &P, v));
    u64* timing = nullptr;
#ifdef ECB_TIMING
    HIPCHK(h, hipMalloc(&timing, ECB_TIMING_WORDS * sizeof(u64)));
    HIPCHK(h, hipMemset(timing, 0, ECB_TIMING_WORDS * sizeof(u64)));
#endif
    h->ctr_synced = false;
    *launched = true;
    const u64 probe_before = h->hctr.n_probe_tiles;
    int rc = ECB_OK;
    for (u32 launch = 0;; ++launch) {
        // records offered to the filter (bam_utils.py:261): all of the batch, once (a relaunch after a park continues the same batch)
        rc = launch_stream(h, v, P, d_rid, d_loc, d_hf, d_pos, n, h->run.prev_rid, d_rid + rec_at(n - 1, tw), launch, launch ? 0 : n, timing);
        if (rc != ECB_OK) break;
        rc = sync_counters(h);
        if (h->prof) {
            float ms = 0; hipEventElapsedTime(&ms, h->ev0, h->ev1);
            h->prof_ms += ms; h->prof_launches += 1;
        }
        if (rc != ECB_OK) break;
        const bool parked = h->hctr.full != 0;
        rc = run_deferred(h, d_rid, d_loc, d_hf, n, false, tw);
        if (rc != ECB_OK) break;
        if (!parked) break;
        rc = grow_table(h, h->cap * 4);                 // some workgroups stopped early: more room, then resume
        if (rc != ECB_OK) break;
    }
#ifdef ECB_TIMING
    {
        u64 t[ECB_TIMING_WORDS];
        hipMemcpy(t, timing, sizeof(t), hipMemcpyDeviceToHost); hipFree(timing);
        static const char* nm[8] = {"(a) filter+heads", "tile decisions", "prefetch issue+clear+geometry", "(b) LDS tables", "hash entries", "(c) lookup", "publish/settle/slot stores", "-"};
        u64 tot = 0; for (int i = 0; i < 7; ++i) tot += t[i];
        fprintf(stderr, "[ecb timing] %llu waves, clocks per wave:", (unsigned long long)P.slices);
        for (int i = 0; i < 7; ++i) fprintf(stderr, "  %s %.0f (%.1f%%)", nm[i], (double)t[i] / P.slices, 100.0 * t[i] / std::max<u64>(tot, 1));
        fprintf(stderr, "  tile visits on the probe-on path %llu of %llu tiles", (unsigned long long)t[7], (unsigned long long)((n + WT - 1) / WT));
        // (c)'s trips to the EC table per lookup of up to 64 reads (a flush; two per flush where a pass holds 128): each is one wait on table memory
        fprintf(stderr, "  table trips per lookup %.3f (claim-only %.3f) over %llu lookups: 1: %.1f%%  2: %.1f%%  3: %.1f%%  4+: %.1f%%", (double)t[12] / std::max<u64>(t[14], 1),
                (double)t[13] / std::max<u64>(t[14], 1), (unsigned long long)t[14], 100.0 * t[8] / std::max<u64>(t[14], 1), 100.0 * t[9] / std::max<u64>(t[14], 1),
                100.0 * t[10] / std::max<u64>(t[14], 1), 100.0 * t[11] / std::max<u64>(t[14], 1));
        // races between waves (k_stream's flush only): claims that found the slot taken since the line was read, by another hash or by a founder with
        // the same; lanes that went through table_settle, and those it sent on to the next slot (the other key of a colliding pair)
        fprintf(stderr, "  [race] claims lost to another hash %llu, to the same hash %llu; lanes in table_settle %llu, of them ST_OTHER %llu",
                (unsigned long long)t[15], (unsigned long long)t[16], (unsigned long long)t[17], (unsigned long long)t[18]);
        fprintf(stderr, "\n");
    }
#endif
    RCCHK(rc);
    {
        const u64 tiles = (n + WT - 1) / WT, on_path = h->hctr.n_probe_tiles - probe_before;
        if (on_path * 4 > tiles) h->par_stream = true; else if (on_path * 16 < tiles) h->par_stream = false;
    }
    if (h->prof) h->prof_records += n;
    if (h->cfg.flags & ECB_F_VERIFY) {                  // belt and braces: the grouping is exact by construction (Slot), this re-derives it
        u64 bad = 0, nl = 0;
        RCCHK(verify_batch(h, d_rid, d_loc, d_hf, n, h->run.prev_rid, &bad, &nl, tw));
        h->run.n_mismatch += bad;
        if (bad) return fail(h, ECB_ERR_VERIFY, "exactness pass: %llu read(s) of this batch sit in an EC whose key is not their target set", (unsigned long long)bad);
    }
    if (hinted) {
        last_rid = h->hctr.last_rid;
        reads_after = (u64)(u32)(last_rid + 1u);
        if (reads_after < h->run.n_reads) return fail(h, ECB_ERR_CONTRACT, "read_id went backwards across pushes");
    }
    h->run.prev_rid = last_rid;
    h->run.n_reads = reads_after;
    h->run.records_pushed += n;
    return ECB_OK;
}
int process_batch(ecb_handle* h, const u32* d_rid, const u32* d_loc, const u32* d_hf, const int* d_pos, u64 n, u32 tw = 512u) {
    bool launched = false;
    const int rc = build_batch(h, d_rid, d_loc, d_hf, d_pos, n, tw, &launched);
    return launched ? run_refused(h, rc) : rc;
}

int ensure_staging(ecb_handle* h, u64 need) {
    if (need <= h->st_cap) return ECB_OK;
    // one allocation for the three (four) staging streams, each on a 2 MiB boundary within it.  (Staging in whole tiles -- what
    // ecb_push_device_tiled takes -- was built and measured: the pitched host-to-device copies cost the PCIe-inclusive rate 8 %, and the
    // tile layout did not take the placement dependence out of the kernel after all: DESIGN.md section 6.)
    h->st_loc = h->st_hf = nullptr; h->st_pos = nullptr; h->st_cap = 0;
    const u64 cap = std::max<u64>(need, h->cfg.max_batch_records);
    const u64 stride = (cap * sizeof(u32) + (2ull << 20) - 1) / (2ull << 20) * (2ull << 20) / sizeof(u32);
    const bool rg = (h->cfg.flags & ECB_F_RANGES) != 0;
    HIPCHK(h, h->st_rid.alloc((rg ? 4 : 3) * stride * sizeof(u32)));
    h->st_cap = cap;
    h->st_loc = h->st_rid + stride; h->st_hf = h->st_rid + 2 * stride;
    if (rg) h->st_pos = reinterpret_cast<int*>(h->st_rid + 3 * stride);
    return ECB_OK;
}

// send carry[0..nc) ++ src[0..m) as one batch
int stage_and_process(ecb_handle* h, const u32* rid, const u32* loc, const u32* hf, const int* pos, u64 m) {
    const u64 nc = h->run.c_rid.size();
    const u64 n = nc + m;
    if (!n) return ECB_OK;
    RCCHK(ensure_staging(h, n));
    const bool rg = (h->cfg.flags & ECB_F_RANGES) != 0;
    // the staged streams {where on the device, the carried read's part, the caller's window}: all the carries are sent, then all the windows
    const struct { void* st; const void *carry, *window; } streams[4] = {
        {h->st_rid, h->run.c_rid.data(), rid}, {h->st_loc, h->run.c_loc.data(), loc}, {h->st_hf, h->run.c_hf.data(), hf}, {h->st_pos, h->run.c_pos.data(), pos}};
    for (int w = 0; w < 2; ++w)
        for (int i = 0; i < (rg ? 4 : 3) && (w ? m : nc); ++i)
            HIPCHK(h, hipMemcpyAsync((u32*)streams[i].st + (w ? nc : 0), w ? streams[i].window : streams[i].carry, (w ? m : nc) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the carry vectors may be rewritten by the caller next
    h->run.c_rid.clear(); h->run.c_loc.clear(); h->run.c_hf.clear(); h->run.c_pos.clear();
    return process_batch(h, h->st_rid, h->st_loc, h->st_hf, rg ? h->st_pos : nullptr, n);
}

// exclusive scan of u32 values, queued on the handle's stream; the sum (64 bits) is left in *d_total on the device
// (a sum of 2^32 or more: the caller's limit check, `out` wrapped)
int excl_scan_dev(ecb_handle* h, const u32* in, u64 n, u32* out, u64* d_total, u32 stride = 1, u32* last32 = nullptr) {
    u32* sums = nullptr;
    POOL(h, P_SUMS, sums, scan_words(n));
    HIPCHK(h, scan_launch(h->stream, in, n, out, sums, d_total, stride, last32));
    return ECB_OK;
}
// ... and with the sum brought to the host (one wait)
int excl_scan(ecb_handle* h, const u32* in, u64 n, u32* out, u64* total) {
    u64* d_tot = nullptr;
    POOL(h, P_TOTALS, d_tot, 8);
    RCCHK(excl_scan_dev(h, in, n, out, d_tot + 7));
    HIPCHK(h, hipMemcpyAsync(total, d_tot + 7, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

// The buffers of a sort of n (key, value) pairs: k[0] / v[0] hold the input; the sort records in `at` which buffer of each pair
// holds its result, and the other one is free.
struct SortBufs {
    u64* k[2];
    u32* v[2];
    int at = 0;
    u64* keys() const { return k[at]; }
    u32* vals() const { return v[at]; }
    u64* spare_keys() const { return k[at ^ 1]; }
    u32* spare_vals() const { return v[at ^ 1]; }
};
// scratch of a sort of n pairs: `hist` = the (tile, digit) words of the look-back, rs_words(n) of them; `offs` = RS_AUX_WORDS words
// (histograms and first places of all passes, the tile counter, the error word); d_word = 8 bytes
struct SortScratch { u32 *hist, *offs; u64* d_word; };
inline u64 rs_tiles(u64 n) { return std::max<u64>(1, (n + RS_TILE - 1) / RS_TILE); }
constexpr u64 RS_AUX_WORDS = 2 * RS_MAX_PASSES * 256 + 64;
inline u64 rs_words(u64 n) { return std::max<u64>(256 * rs_tiles(n), RS_AUX_WORDS); }
// Stable LSD radix sort of n (key, value) pairs on `st`: only the digits some key has a bit in are sorted on (one OR-reduction
// and one host wait up front, unless bit_mask names them).
hipError_t radix_sort_pairs64(hipStream_t st, SortBufs& b, u64 n, const SortScratch& sc, u64 bit_mask = ~0ull) {
    b.at = 0;
    if (n < 2) return hipSuccess;
    if (n >= (1ull << 30)) return hipErrorInvalidValue;          // (a look-back word carries a 30-bit count)
    hipError_t e = hipSuccess;
    u64 ormask = bit_mask;                          // (a caller that names the bits to sort on has no use for the reduction and its host wait)
    if (bit_mask == ~0ull) {
        if ((e = hipMemsetAsync(sc.d_word, 0, 8, st)) != hipSuccess) return e;
        k_or_reduce<<<(unsigned)std::min<u64>(1024, (n + TPB - 1) / TPB), TPB, 0, st>>>(b.k[0], n, sc.d_word);
        if ((e = hipMemcpyAsync(&ormask, sc.d_word, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    }
    RsShifts sh{};
    for (u32 shift = 0; shift < 64; shift += 8)
        if ((ormask >> shift) & 255ull) sh.s[sh.n++] = shift;   // (every key has zero in the other digits: already in order)
    if (!sh.n) return hipSuccess;
    const u32 nt = (u32)rs_tiles(n);
    u32 *ghist = sc.offs, *base = sc.offs + RS_MAX_PASSES * 256, *ticket = sc.offs + 2 * RS_MAX_PASSES * 256, *err = ticket + 1;
    if ((e = hipMemsetAsync(sc.offs, 0, RS_AUX_WORDS * 4, st)) != hipSuccess) return e;
    k_rs_hist_all<<<(unsigned)std::min<u64>(2048, (n + 16 * RS_TPB - 1) / (16 * RS_TPB)), RS_TPB, 0, st>>>(b.k[0], n, sh, ghist);
    k_rs_bases<<<1, 256, 0, st>>>(ghist, sh.n, base);
    for (u32 p = 0; p < sh.n; ++p) {
        if ((e = hipMemsetAsync(sc.hist, 0, (u64)nt * 256 * 4, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(ticket, 0, 4, st)) != hipSuccess) return e;
        k_rs_pass<<<nt, RS_TPB, 0, st>>>(b.keys(), b.vals(), n, sh.s[p], base + p * 256, sc.hist, ticket, err, b.spare_keys(), b.spare_vals());
        b.at ^= 1;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    u32 gave_up = 0;                                // (a look-back that ran out of polls leaves the order undefined: never silently)
    if ((e = hipMemcpyAsync(&gave_up, err, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    return gave_up ? hipErrorUnknown : hipSuccess;
}
// ... on the handle's stream, with its pool's scratch
int handle_sort(ecb_handle* h, SortBufs& b, u64 n, u64 bit_mask = ~0ull) {
    SortScratch sc{};
    u64* tot = nullptr;
    POOL(h, P_RS_HIST, sc.hist, rs_words(n)); POOL(h, P_RS_OFFS, sc.offs, RS_AUX_WORDS); POOL(h, P_TOTALS, tot, 8);
    sc.d_word = tot + 6;
    HIPCHK_AS(h, "radix sort: ", radix_sort_pairs64(h->stream, b, n, sc, bit_mask));
    return ECB_OK;
}
// ... and its runs of equal keys: flag[i] = 1 where one starts, pos = the exclusive scan of the flags, *n_runs their number (one wait)
int sorted_runs(ecb_handle* h, SortBufs& b, u64 n, u32* flag, u32* pos, u64* n_runs) {
    RCCHK(handle_sort(h, b, n));
    k_run_heads<<<nblk(n, TPB), TPB, 0, h->stream>>>(b.keys(), n, flag);
    return excl_scan(h, flag, n, pos, n_runs);
}

int ensure_slot_ranks(ecb_handle* h, u64 E) {
    if (h->run.csr.rank_of_slot) return ECB_OK;                     // (null: not made yet)
    POOL(h, P_RANK, h->run.csr.rank_of_slot, h->cap);
    k_slot_ranks<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->run.csr.order, E, h->run.csr.rank_of_slot);
    HIPCHK(h, hipGetLastError());
    return ECB_OK;
}

// reads per EC / first appearance, from read_slot[0, n_reads) (once, when the stream is closed).  Only queues kernels:
// the totals and the work list of k_count_bins stay on the device.  *listed (finalize's): k_count_bins filled the caller's sink as it went.
int ensure_counts(ecb_handle* h, const CompactSink* sink = nullptr, bool* listed = nullptr) {
    if (h->counted()) return ECB_OK;
    const u64 R = h->run.n_reads;
    CompactSink own{nullptr, 0, nullptr, nullptr, 0, nullptr};
    if (R && !sink && h->run.origin != Origin::ADOPTED && h->n_ecs()) {         // (a table export follows: it wants the list of occupied slots, see k_count_bins)
        u32* list = nullptr;
        u64* d_n = nullptr;
        POOL(h, P_LIST, list, h->n_ecs());
        POOL(h, P_CNT, d_n, 1);
        HIPCHK(h, hipMemsetAsync(d_n, 0, sizeof(u64), h->stream));
        own = CompactSink{list, h->n_ecs(), d_n, nullptr, 0, nullptr};
        sink = &own;
    }
    if (R) {
        // Slots per range: 512 ranges -- one k_count_bins workgroup for each of the chip's 512 places, all at once -- unless that takes more than 2^14 slots
        // each (64 KB of LDS counters: two workgroups per CU; 2^15 leaves room for one).  C3: 1 024 ranges of 2^14; C2: 512 of 2^13; the diploid stream
        // 512 of 2^13.  Fewer, fuller ranges leave CUs without a workgroup (C2 with 256 ranges: k_count_bins 0.19 ms against 0.13); more ranges make the
        // partition's runs shorter (k_part_scatter_staged at C3 with 2 048: 0.38 ms against 0.26; on the diploid stream with 2 048: 0.71 against 0.49 with 1 024)
        // -- profiles/r04_finalize_kernels.txt.
        u32 bb = BIN_BITS;
        {
            u32 lc = 0;
            while ((1ull << (lc + 1)) <= h->cap) ++lc;   // the table holds 2^lc slots
            bb = std::min<u32>(std::max<u32>(lc, 9u + MIN_BIN_BITS) - 9u, BIN_BITS);
        }
        if (const char* e = getenv("ECB_BIN_BITS")) bb = (u32)std::min<long>(std::max<long>(atol(e), MIN_BIN_BITS), MAX_BIN_BITS);   // (measurement knob: tools/tools_env.sh)
        while (bb < MAX_BIN_BITS && (h->cap >> bb) > MAX_BUCKETS) ++bb;
        const u32 nb = (u32)std::max<u64>(1, h->cap >> bb);
        if (nb > MAX_BUCKETS) return fail(h, ECB_ERR_LIMIT, "EC table larger than 2^28 slots is not supported");
        if (bb > 14 && !h->count_attr_set) {        // (more than 64 KB of dynamic LDS has to be asked for)
            HIPCHK(h, hipFuncSetAttribute((const void*)k_count_bins, hipFuncAttributeMaxDynamicSharedMemorySize, 4 << MAX_BIN_BITS));
            h->count_attr_set = true;
        }
        const u32 G = (u32)std::min<u64>(PART_G, (R + 4095) / 4096);
        u32 *hist = nullptr, *offs = nullptr;
        u16* pairs = nullptr;
        u64* d_tot = nullptr;
        POOL(h, P_HIST, hist, (u64)nb * G); POOL(h, P_OFFS, offs, (u64)nb * G);
        POOL(h, P_PAIRS, pairs, R);
        POOL(h, P_TOTALS, d_tot, 8);
        k_part_hist<<<G, TPB_PART, nb * 4, h->stream>>>(h->read_slot, R, nb, bb, hist);
        d_tot += 6;                                 // ([0..3] are finalize's, which may run this with its own totals already zeroed; [7] is excl_scan's)
        RCCHK(excl_scan_dev(h, hist, (u64)nb * G, offs, d_tot));
        if (nb <= STAGE_MAX_BUCKETS) {
            if (!h->scatter_attr_set) {             // (per handle = per device: more than 64 KB of dynamic LDS has to be asked for)
                HIPCHK(h, hipFuncSetAttribute((const void*)k_part_scatter_staged, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              3 * STAGE_MAX_BUCKETS * 4 + STAGE * 4));
                h->scatter_attr_set = true;
            }
            k_part_scatter_staged<<<G, TPB_PART, 3 * nb * 4 + STAGE * 4, h->stream>>>(h->read_slot, R, nb, bb, offs, pairs);
        } else                                     // (tables beyond 2^25 slots: the counters would crowd the stage out of LDS)
            k_part_scatter<<<G, TPB_PART, nb * 4, h->stream>>>(h->read_slot, R, nb, bb, offs, pairs);
        // work list of k_count_bins: ranges far above the average are cut into pieces (see CountWork)
        const u32 piece = std::max<u32>(32768u, 2u * (u32)((R + nb - 1) / nb));
        const u32 max_work = nb + (u32)(R / piece) + 1;
        CountWork* d_work = nullptr;
        POOL(h, P_WORK, d_work, (u64)max_work + 1);          // (+ 1: its length sits behind the list)
        u32* d_nwork = reinterpret_cast<u32*>(d_work + max_work);
        k_build_work<<<1, 1024, 0, h->stream>>>(offs, G, d_tot, nb, piece, d_work, max_work, d_nwork);
        k_count_bins<<<max_work, TPB_COUNT, 4u << bb, h->stream>>>(pairs, d_work, d_nwork, bb, h->table, sink ? *sink : CompactSink{nullptr, 0, nullptr, nullptr, 0, nullptr});
        if (sink == &own) h->run.d_list_n = own.n_list;
        else if (sink && listed) *listed = true;
        HIPCHK(h, hipGetLastError());
    }
    h->run.stage = Stage::COUNTED;
    return ECB_OK;
}

// occupied slots -> pool[P_LIST] (+ first-appearance bitmap and (first, key length) per entry for finalize); the number found
// is left in *d_n on the device
int compact_table_dev(ecb_handle* h, u64* d_n, u32* bitmap = nullptr, u64 n_bits = 0, uint2* list_fn = nullptr) {
    u32* list = nullptr;
    HIPCHK(h, hipMemsetAsync(d_n, 0, sizeof(u64), h->stream));
    POOL(h, P_LIST, list, h->n_ecs());
    k_compact<<<(unsigned)std::min<u64>(2048, (h->cap + 4 * TPB_COMPACT - 1) / (4 * TPB_COMPACT)), TPB_COMPACT, 0, h->stream>>>(h->table, h->cap, list, std::max<u64>(h->n_ecs(), 1), d_n, bitmap, n_bits, list_fn);
    return ECB_OK;
}
int compact_table(ecb_handle* h) {
    u64* d_n = h->run.d_list_n;                          // the counting pass listed them: no scan of the table
    if (!d_n) {
        POOL(h, P_CNT, d_n, 1);
        RCCHK(compact_table_dev(h, d_n));
    }
    HIPCHK(h, hipMemcpyAsync(&h->run.n_list, d_n, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->run.n_list != h->n_ecs()) return fail(h, ECB_ERR_HIP, "internal: %llu occupied slots but %llu ECs created",
                                             (unsigned long long)h->run.n_list, (unsigned long long)h->n_ecs());
    return ECB_OK;
}

// distinct (EC, cell, file) triples of this handle's reads: sort the per-read keys (EC id << 32 | meta), run-length encode.
// ec_of_slot maps a table slot to the EC id to use (the handle's own ranks, or global ranks in a multi-GPU run).
int ms_reduce(ecb_handle* h, const u32* ec_of_slot) {
    const u64 R = h->run.n_reads;
    if (h->run.meta_hi < R) return fail(h, ECB_ERR_STATE, "ecb_push_cells covered %llu of %llu reads",
                                    (unsigned long long)h->run.meta_hi, (unsigned long long)R);
    u64 *keys = nullptr, *keys2 = nullptr; u32 *vals = nullptr, *vals2 = nullptr, *flag = nullptr, *pos = nullptr;
    POOL(h, P_MS_KEYS, keys, R); POOL(h, P_MS_KEYS2, keys2, R); POOL(h, P_MS_VALS, vals, R); POOL(h, P_MS_VALS2, vals2, R);
    POOL(h, P_MS_FLAG, flag, R); POOL(h, P_MS_POS, pos, R);
    k_ms_keys<<<nblk(R, TPB), TPB, 0, h->stream>>>(h->read_slot, ec_of_slot, h->meta, R, keys, vals);
    SortBufs s{{keys, keys2}, {vals, vals2}};
    u64 nt = 0;
    RCCHK(sorted_runs(h, s, R, flag, pos, &nt));
    POOL(h, P_MS_OKEY, h->run.tri.okey, nt); POOL(h, P_MS_OFIRST, h->run.tri.ofirst, nt); POOL(h, P_MS_OSTART, h->run.tri.ostart, (u64)nt + 1);
    k_ms_emit<<<nblk(R, TPB), TPB, 0, h->stream>>>(s.keys(), s.vals(), flag, pos, R, nt, h->run.tri.okey, h->run.tri.ofirst, h->run.tri.ostart);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->run.tri.n = nt; h->run.tri.ocount = nullptr; h->run.triples = Triples::OWN;
    return ECB_OK;
}

// exported entries number their first reads from the shard's own 0 (or from the read_base given at export): move them on by `base`
__global__ void k_rebase(Entry* e, u64 n, u32 base, u32 limit, Counters* ctr) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 first = ~e[i].first_inv;
    if (first >= limit) { atomicOr(&ctr->err, ERR_CONTRACT); return; }     // (would run past 2^32 - 2 reads)
    e[i].first_inv = ~(first + base);
}

// ---- finalize per key range (multi-GPU): every rank ranks and emits the ECs of its own key range, the root only puts the pieces
// in the order of first appearance.  The rank of an EC = the number of ECs whose first read comes before its own
// (bam_utils.py:682-698): a bitmap over the reads, marked from every piece's first reads, and its prefix popcount.
__global__ void k_export_firsts(const Slot* table, const u32* order, u64 n, u32* firsts) {
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e < n) firsts[e] = ~table[order[e]].first_inv;
}
struct PieceDesc { const u32* firsts; const int *indptr, *indices, *data, *counts; u64 n, nnz, at; };   // one finalized key range (at: its first EC among all pieces')
// (all pieces in one launch: blockIdx.y = piece)
__global__ void k_mark_bits(const PieceDesc* P, u64 n_bits, u32* bitmap, Counters* ctr) {
    const PieceDesc d = P[blockIdx.y];
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= d.n) return;
    const u32 f = d.firsts[e];
    if (f >= n_bits) { atomicOr(&ctr->err, ERR_CONTRACT); return; }
    atomicOr(&bitmap[f >> 5], 1u << (f & 31u));
}
// (what is known of rank r goes out as ONE 16-byte word {EC within its piece + 1, row length, count, piece}: the scatter is this kernel's cost)
__global__ void k_piece_place(const PieceDesc* P, u64 n_total, u64 n_bits, const u32* bitmap, const u32* wprefix, uint4* place, Counters* ctr) {
    const PieceDesc d = P[blockIdx.y];
    const u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (e >= d.n) return;
    const u32 f = d.firsts[e];
    if (f >= n_bits) return;                             // (reported by k_mark_bits)
    const long long s0 = d.indptr[e], s1 = d.indptr[e + 1];
    if (s0 < 0 || s1 < s0 || (u64)s1 > d.nnz) { atomicOr(&ctr->err, ERR_CONTRACT); return; }
    const u32 r = bit_rank(bitmap, wprefix, f);
    if (r >= n_total) return;
    const u32 cnt = (u32)d.counts[e];
    if (cnt > 0x7FFFFFFFu) atomicOr(&ctr->err, ERR_COUNT);     // (an entry of N is an int32)
    place[r] = make_uint4((u32)e + 1u, (u32)(s1 - s0), cnt, blockIdx.y);    // (two pieces claiming one first read: either, whole; the caller reports it)
}
// One thread per row of the result: neighbours write neighbouring rows, and read rows that follow each other within their piece
// (a piece is in first-read order itself).
__global__ void k_piece_rows(const PieceDesc* P, u32 n_pieces, const uint4* place, u64 n_total, const u32* indptr, int* indices, int* data, int* counts) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r >= n_total) return;
    const uint4 pl = place[r];
    counts[r] = (int)pl.z;
    if (pl.x == 0u || pl.w >= n_pieces) return;         // (no piece claimed this rank: the caller reports it)
    const u32 q = pl.w;
    const u64 e = pl.x - 1u;
    const int* ip = P[q].indptr;
    const int s0 = ip[e], s1 = ip[e + 1];
    const u32 d0 = indptr[r];
    if (indptr[r + 1] - d0 != (u32)(s1 - s0) || pl.y != (u32)(s1 - s0)) return;   // (nothing is ever written past a row)
    const int *sj = P[q].indices, *sd = P[q].data;
    for (int i = s0; i < s1; ++i) { indices[d0 + (u32)(i - s0)] = sj[i]; data[d0 + (u32)(i - s0)] = sd[i]; }
}

// ---- what entry points share -----------------------------------------------------------------------------------------------------------
// the three pushes: a handle, a stream that still takes records, and the records themselves
int push_refused(ecb_handle* h, size_t n, bool streams_given) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->can_push()) return fail(h, ECB_ERR_STATE, "push after finalize / table export");
    if (n && !streams_given) return fail(h, ECB_ERR_ARG, "null tuple stream");
    return ECB_OK;
}
// ... and the two that take device memory (ptr_bits: their pointers, or-ed)
int device_push_refused(ecb_handle* h, const char* who, uintptr_t ptr_bits) {
    if (ptr_bits & 15) return fail(h, ECB_ERR_ARG, "device streams must be 16-byte aligned");
    if (h->open_read()) return fail(h, ECB_ERR_STATE, "%s while a host push has an open read", who);
    HIPCHK(h, hipSetDevice(h->device));
    return ECB_OK;
}
// ecb_verify_device / ecb_verify_device_tiled: the exactness pass over one batch, as three streams or as tiles (tw: verify_batch)
int verify_streams(ecb_handle* h, const void* d_rid, const void* d_loc, const void* d_hf, size_t n, u32 tw, u64* n_mismatch, u64* n_long) {
    RCCHK(refused_run(h));
    if (!n || !d_rid || !d_loc || !d_hf) return fail(h, ECB_ERR_ARG, "null tuple stream");
    if (((uintptr_t)d_rid | (uintptr_t)d_loc | (uintptr_t)d_hf) & 15) return fail(h, ECB_ERR_ARG, "device streams must be 16-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    return verify_batch(h, (const u32*)d_rid, (const u32*)d_loc, (const u32*)d_hf, n, 0xFFFFFFFFu, n_mismatch, n_long, tw);
}
// ecb_push_cells / ecb_push_cells_device: meta of reads [first_read, first_read + n), from the host or from device memory (`kind`)
int push_cells(ecb_handle* h, const void* meta, uint64_t first_read, size_t n, hipMemcpyKind kind) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->multisample()) return fail(h, ECB_ERR_STATE, "handle was created without ECB_F_MULTISAMPLE");
    if (h->has_result()) return fail(h, ECB_ERR_STATE, "push after finalize");
    if (!n) return ECB_OK;
    if (!meta) return fail(h, ECB_ERR_ARG, "null meta");
    HIPCHK(h, hipSetDevice(h->device));
    if (first_read >= (1ull << 32) - 1 || (u64)n >= (1ull << 32) - 1 - first_read) return fail(h, ECB_ERR_LIMIT, "more than 2^32-2 reads");
    const u64 need = first_read + n;
    RCCHK(ensure_meta(h, need));
    // (from device memory: ordered on the handle's own stream, behind nothing of the caller's: it must be COMPLETE when this is called -- see
    //  ecb.h -- and nothing is waited for; from the host: the caller may rewrite its array next)
    HIPCHK(h, hipMemcpyAsync(h->meta + first_read, meta, n * sizeof(u32), kind, h->stream));
    if (kind == hipMemcpyHostToDevice) HIPCHK(h, hipStreamSynchronize(h->stream));
    h->run.meta_hi = std::max<u64>(h->run.meta_hi, need);
    return ECB_OK;
}
// ecb_finalize / ecb_assemble_ranges_device: what neither builds a result from ...
int refuse_no_ecs(ecb_handle* h, u64 E, u64 valid) {
    if (E == 0 || valid == 0) return fail(h, ECB_ERR_EMPTY, "no valid alignments: nothing to build (the reference fails here too)");
    if (E >= (1ull << 31) - 1) return fail(h, ECB_ERR_LIMIT, "more than 2^31-2 equivalence classes");
    return ECB_OK;
}
int refuse_nnz(ecb_handle* h, u64 nnz) {
    if (nnz >= (1ull << 31)) return fail(h, ECB_ERR_LIMIT, "A has more than 2^31-1 non-zeros");
    return ECB_OK;
}
// ... and the sizes of what they built: one sample, N = the count of every EC (a multisample handle then says what its N is)
ecb_sizes result_sizes(u64 E, u64 nnz, u64 all, u64 valid, u64 reads) {
    ecb_sizes s{};
    s.n_ecs = E; s.nnz_a = nnz; s.n_samples = 1; s.nnz_n = E;
    s.all_alignments = all; s.valid_alignments = valid; s.n_reads = reads;
    return s;
}
// ecb_export / ecb_export_device: A's three arrays and the counts are copied out on the stream (`kind`: to the host, or within the device);
// N's other two arrays are trivial -- one column: {0, E} and 0 .. E-1 -- and written where the output lives
int export_result(ecb_handle* h, void* ia, void* ja, void* da, void* in_, void* jn, void* dn, hipMemcpyKind kind) {
    HIPCHK(h, hipSetDevice(h->device));
    const bool on_device = kind == hipMemcpyDeviceToDevice;
    const u64 E = h->run.sizes.n_ecs, nnz = h->run.sizes.nnz_a;
    const ecb_handle::Run::Csr& r = h->run.csr;
    if (ia) HIPCHK(h, hipMemcpyAsync(ia, r.indptr, (E + 1) * 4, kind, h->stream));
    if (ja) HIPCHK(h, hipMemcpyAsync(ja, r.indices, nnz * 4, kind, h->stream));
    if (da) HIPCHK(h, hipMemcpyAsync(da, r.data, nnz * 4, kind, h->stream));
    if (on_device) {
        if (in_) { const int v[2] = {0, (int)E}; HIPCHK(h, hipMemcpyAsync(in_, v, 8, hipMemcpyHostToDevice, h->stream)); }
        if (jn) k_iota<<<nblk(E, TPB), TPB, 0, h->stream>>>((u32*)jn, E);
    }
    if (dn) HIPCHK(h, hipMemcpyAsync(dn, r.counts, E * 4, kind, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!on_device) {
        if (in_) { ((int32_t*)in_)[0] = 0; ((int32_t*)in_)[1] = (int32_t)E; }
        if (jn) for (u64 i = 0; i < E; ++i) ((int32_t*)jn)[i] = (int32_t)i;
    }
    return ECB_OK;
}

}  // namespace

extern "C" {

int ecb_abi_version(void) { return ECB_ABI_VERSION; }

int ecb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ecb_last_error(const ecb_handle* h) { return h ? h->err.c_str() : t_err.c_str(); }

int ecb_create(const ecb_config* cfg, ecb_handle** out) {
    if (!cfg || !out || cfg->struct_size != sizeof(ecb_config)) return fail(nullptr, ECB_ERR_ARG, "bad ecb_config (struct_size)");
    if (cfg->n_loci == 0 || cfg->n_loci >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "n_loci out of range (1 .. 2^26-3)");
    if (cfg->n_haplotypes == 0 || cfg->n_haplotypes > 31) return fail(nullptr, ECB_ERR_ARG, "n_haplotypes must be 1..31 (A stores a bitmask in int32)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, ECB_ERR_NO_DEVICE, "no HIP device: libecb has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, ECB_ERR_ARG, "device %d out of range (%d present)", cfg->device, ndev);
    std::unique_ptr<ecb_handle> owner(new ecb_handle());  // (an early return frees what was built so far)
    ecb_handle* const h = owner.get();
    h->cfg = *cfg;
    h->device = cfg->device;
    if (!h->cfg.ec_capacity) h->cfg.ec_capacity = 1ull << 22;
    if (!h->cfg.arena_capacity) h->cfg.arena_capacity = 1ull << 26;
    if (!h->cfg.max_batch_records) h->cfg.max_batch_records = 1ull << 24;
    h->cap = std::max<u64>(next_pow2(h->cfg.ec_capacity), 1024);
    h->arena_cap = std::min<u64>(h->cfg.arena_capacity, 1ull << 32);
#define CREATECHK(call) HIPCHK_AS(nullptr, "ecb_create: ", call)      // (the text of a handle that is about to go would go with it)
    CREATECHK(hipSetDevice(h->device));
    CREATECHK(hipStreamCreate(&h->stream));
    CREATECHK(h->table.alloc(h->cap * sizeof(Slot)));
    CREATECHK(h->arena.alloc(h->arena_cap * sizeof(uint2)));
    CREATECHK(h->ctr.alloc(sizeof(Counters)));
    CREATECHK(pin(h->pin_ctr));
    CREATECHK(pin(h->pin_cold));
    CREATECHK(pin(h->pin_out));
    CREATECHK(h->d_cold.alloc(sizeof(StreamCold)));
    CREATECHK(hipMemsetAsync(h->table, 0, h->cap * sizeof(Slot), h->stream));
    CREATECHK(hipMemsetAsync(h->arena, 0, h->arena_cap * sizeof(uint2), h->stream));     // stale arena bytes must never look like a key (see ecb_reset)
    if (const int rc = clear_counters(h); rc != ECB_OK) return fail(nullptr, rc, "ecb_create: %s", h->err.c_str());
    if (cfg->flags & ECB_F_RANGES) {
        const u64 ns = (u64)cfg->n_loci * cfg->n_haplotypes;
        CREATECHK(h->rng.alloc(ns * sizeof(int2)));
        k_fill_minmax<<<nblk(ns, TPB), TPB, 0, h->stream>>>(h->rng, ns);
    }
    hipEventCreate(&h->ev0); hipEventCreate(&h->ev1);
    CREATECHK(hipStreamSynchronize(h->stream));
#undef CREATECHK
    *out = owner.release();
    return ECB_OK;
}

void ecb_destroy(ecb_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    delete h;                                            // (the events and the stream, then the memory the handle owns)
}

int ecb_verify_device(ecb_handle* h, const void* d_read_id, const void* d_locus, const void* d_hapflag, size_t n,
                      uint64_t* n_mismatch, uint64_t* n_long) {
    if (!h || !n_mismatch || !n_long) return ECB_ERR_ARG;
    u64 bad = 0, nl = 0;
    const int rc = verify_streams(h, d_read_id, d_locus, d_hapflag, n, 512u, &bad, &nl);
    *n_mismatch = bad; *n_long = nl;
    return rc;
}

int ecb_reset(ecb_handle* h) {
    if (!h) return ECB_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const u32* occupied = h->has_result() ? h->slot_list() : nullptr;     // (a finalized handle knows its occupied slots: every one of them, checked)
    const u64 n_occupied = h->run.n_list;
    // ECB_POISON_SCRATCH: the run's scratch is dead from here on (run = Run{} below drops every view into it).  Not the two buffers k_slow
    // leaves zeroed for its next launch (run_slow clears them only when they are reallocated), and the list of occupied slots only once
    // the table has been cleared from it.  The table, the arena, read_slot, meta, the queue and the wave arena are no scratch: what of them a
    // reset clears, it clears by its own rule below.
    const bool poison = poison_scratch();
    if (poison)
        for (int i = 0; i < ecb_handle::P_N; ++i)
            if (h->pool[i].p && i != ecb_handle::P_SLOW_KEY && i != ecb_handle::P_SLOW_MASK && i != ecb_handle::P_LIST)
                HIPCHK(h, hipMemsetAsync(h->pool[i].p, POISON_BYTE, h->pool[i].bytes, h->stream));
    // The used stretches of the key arena go back to zero: a key pair is only ever compared against bytes that are either
    // zero (no haplotype mask: never equal to a pair) or final, whatever a cache still holds of them.
    if (!h->ctr_synced) sync_counters(h);               // (the cursors; an error the run already reported is not this call's)
    {   // (one launch for all of them: a fill per region was 64 dispatches of ~5 us on a stream with long keys -- the paralog stream's reset 0.3 ms)
        const u32 R = arena_regions(h->arena_cap);
        const u64 per = h->arena_cap / R;
        ArenaClear ac{};
        u32 n = 0;
        u64 longest = 0;
        for (u32 r = 0; r < R; ++r) {
            const u64 used = std::min<u64>(h->hctr.arena_reg[r], (u64)(r + 1) * per) - r * per;
            if (used) { ac.start[n] = r * per; ac.len[n] = used; ++n; longest = std::max(longest, used); }
        }
        if (h->hctr.arena_top) { ac.start[n] = 0; ac.len[n] = std::min<u64>(h->hctr.arena_top, h->arena_cap); longest = std::max(longest, ac.len[n]); ++n; }
        if (n) {
            const dim3 grid((unsigned)std::min<u64>(nblk(longest, TPB), 2048), n);
            k_clear_arena<<<grid, TPB, 0, h->stream>>>(h->arena, ac);
            HIPCHK(h, hipGetLastError());
        }
    }
#if defined(ECB_TIMING) || defined(ECB_EXPERIMENTS)     // experiment builds only (tools/exp_hits.py: a pass over a table that holds every EC already)
    if (!getenv("ECB_KEEP_TABLE"))
#endif
    {
        // a sparsely filled table is cleared slot by slot from that list (config 3: 3.7 M of 16.8 M slots, 0.24 of 1 GB)
        if (h->run.origin == Origin::ASSEMBLED) {
            // (a result assembled from per-range pieces never touched this handle's table)
        } else if (occupied && n_occupied && n_occupied == h->n_ecs() && !h->hctr.err && n_occupied * 3 < h->cap)
            k_clear_slots<<<nblk(n_occupied, TPB), TPB, 0, h->stream>>>(h->table, occupied, n_occupied);
        else
            HIPCHK(h, hipMemsetAsync(h->table, 0, h->cap * sizeof(Slot), h->stream));
    }
    if (poison && h->pool[ecb_handle::P_LIST].p)
        HIPCHK(h, hipMemsetAsync(h->pool[ecb_handle::P_LIST].p, POISON_BYTE, h->pool[ecb_handle::P_LIST].bytes, h->stream));
    RCCHK(clear_counters(h));
    if (h->wave_arena) HIPCHK(h, hipMemsetAsync(h->wave_arena, 0, 2 * h->wave_arena_n * sizeof(u64), h->stream));
    // (read_slot keeps the last run's slot ids: every read of the next stream has its entry written by k_stream or k_slow
    //  before anything reads it -- k_count, the exports and the exactness pass look at reads [0, n_reads) of a stream that was
    //  looked up without an error -- and entries of a fresh allocation are PENDING.  384 MB of stores per run at config 3.
    //  A handle that checks itself (ECB_F_VERIFY) pays for the fill: a read the stream kernel skipped then shows as PENDING, which the
    //  exactness pass counts as a read in a wrong EC.)
    if ((h->cfg.flags & ECB_F_VERIFY) && h->read_slot) HIPCHK(h, hipMemsetAsync(h->read_slot, 0xFF, h->read_slot_cap * sizeof(u32), h->stream));
    if (h->rng) {
        const u64 ns = (u64)h->cfg.n_loci * h->cfg.n_haplotypes;
        k_fill_minmax<<<nblk(ns, TPB), TPB, 0, h->stream>>>(h->rng, ns);
    }
    // (no wait: everything above is ordered on the handle's stream, where all later work goes too)
    h->run = ecb_handle::Run{};
    h->err.clear();                                     // (the text of a refusal goes with the run it was about)
    return ECB_OK;
}

int ecb_hint_reads(ecb_handle* h, uint64_t max_reads) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (max_reads >= (1ull << 32)) return fail(h, ECB_ERR_LIMIT, "more than 2^32 - 1 reads");
    h->reads_hint = max_reads;
    return ECB_OK;
}

int ecb_push_device(ecb_handle* h, const void* d_read_id, const void* d_locus, const void* d_hapflag,
                    const void* d_pos, size_t n) {
    RCCHK(push_refused(h, n, d_read_id && d_locus && d_hapflag));
    if ((h->cfg.flags & ECB_F_RANGES) && n && !d_pos) return fail(h, ECB_ERR_ARG, "ECB_F_RANGES needs pos");
    RCCHK(device_push_refused(h, "ecb_push_device", (uintptr_t)d_read_id | (uintptr_t)d_locus | (uintptr_t)d_hapflag | (uintptr_t)d_pos));
    return process_batch(h, (const u32*)d_read_id, (const u32*)d_locus, (const u32*)d_hapflag, (const int*)d_pos, n);
}

// The same from ONE buffer of whole tiles: tile t = words [1536 t, 1536 t + 1536) = 512 read ids | 512 loci | 512 haplotype/flag words of records
// [512 t, 512 t + 512) (the last tile padded: the buffer holds ceil(n / 512) tiles).  What a tile of the stream kernel reads is then 6 KB in one
// place instead of 2 KB in each of three.  (Built to take the kernel's dependence on where the streams sit in HBM out -- a micro-benchmark of the
// reads alone said three streams side by side were the sensitive part -- and measured: it narrows the spread, 7.7 - 8.7 ms against 7.7 - 9.3 on
// config 3, but does not remove it: DESIGN.md section 6.  Kept as a second way in for callers whose tuples sit in one buffer.)
int ecb_push_device_tiled(ecb_handle* h, const void* d_tiles, size_t n) {
    RCCHK(push_refused(h, n, d_tiles != nullptr));
    if (h->cfg.flags & ECB_F_RANGES) return fail(h, ECB_ERR_STATE, "ECB_F_RANGES takes the four streams of ecb_push_device");
    RCCHK(device_push_refused(h, "ecb_push_device_tiled", (uintptr_t)d_tiles));
    const u32* d = (const u32*)d_tiles;
    return process_batch(h, d, d + 512, d + 1024, nullptr, n, 1536u);
}

int ecb_verify_device_tiled(ecb_handle* h, const void* d_tiles, size_t n, uint64_t* n_mismatch, uint64_t* n_long_reads) {
    if (!h || !n_mismatch) return ECB_ERR_ARG;
    u64 bad = 0, nl = 0;
    const u32* d = (const u32*)d_tiles;
    RCCHK(verify_streams(h, d, d ? d + 512 : d, d ? d + 1024 : d, n, 1536u, &bad, &nl));
    *n_mismatch = bad;
    if (n_long_reads) *n_long_reads = nl;
    return ECB_OK;
}

int ecb_push(ecb_handle* h, const uint32_t* rid, const uint32_t* loc, const uint32_t* hf, const int32_t* pos, size_t n) {
    RCCHK(push_refused(h, n, rid && loc && hf));
    const bool rg = (h->cfg.flags & ECB_F_RANGES) != 0;
    if (rg && n && !pos) return fail(h, ECB_ERR_ARG, "ECB_F_RANGES needs pos");
    HIPCHK(h, hipSetDevice(h->device));
    u64 done = 0;
    while (done < n) {
        const u64 m = std::min<u64>(h->cfg.max_batch_records, n - done);
        const u32 *r = rid + done, *l = loc + done, *f = hf + done;
        const int* ps = rg ? pos + done : nullptr;
        // records [cut, m) share the window's last read_id: that read may continue in the next push
        const u32 last = r[m - 1];
        u64 cut = m;
        while (cut > 0 && r[cut - 1] == last) --cut;
        const bool carry_continues = !h->run.c_rid.empty() && h->run.c_rid.back() == last;
        if (cut == 0 && (carry_continues || h->run.c_rid.empty())) {
            h->run.c_rid.insert(h->run.c_rid.end(), r, r + m);
            h->run.c_loc.insert(h->run.c_loc.end(), l, l + m);
            h->run.c_hf.insert(h->run.c_hf.end(), f, f + m);
            if (rg) h->run.c_pos.insert(h->run.c_pos.end(), ps, ps + m);
        } else {
            RCCHK(stage_and_process(h, r, l, f, ps, cut));      // carry ++ window[0, cut): whole reads
            h->run.c_rid.assign(r + cut, r + m);
            h->run.c_loc.assign(l + cut, l + m);
            h->run.c_hf.assign(f + cut, f + m);
            if (rg) h->run.c_pos.assign(ps + cut, ps + m);
        }
        done += m;
    }
    return ECB_OK;
}

int ecb_push_cells(ecb_handle* h, const uint32_t* meta, uint64_t first_read, size_t n) {
    return push_cells(h, meta, first_read, n, hipMemcpyHostToDevice);
}

int ecb_push_cells_device(ecb_handle* h, const void* d_meta, uint64_t first_read, size_t n) {
    return push_cells(h, d_meta, first_read, n, hipMemcpyDeviceToDevice);
}

int ecb_finalize(ecb_handle* h, ecb_sizes* out) {
    if (!h || !out) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (h->run.origin == Origin::ASSEMBLED) { *out = h->run.sizes; return ECB_OK; }   // (the result of ecb_assemble_ranges_device: nothing left to rank)
    if (!h->has_result()) {
        if (h->open_read()) RCCHK(stage_and_process(h, nullptr, nullptr, nullptr, nullptr, 0));   // the stream ends here: the carried read is complete
        if (!h->ctr_synced) RCCHK(sync_counters(h));
    }
    const u64 E = h->n_ecs();
    const u64 valid = h->hctr.valid + h->run.extra_valid;
    RCCHK(refuse_no_ecs(h, E, valid));
    h->run.csr = {};                                 // (rank_of_slot: made on demand, ensure_slot_ranks)
    // Everything below is queued on the stream; the host waits once, at the end, and checks what the device counted.
    // rank by first appearance: bitmap over read indices (marked while the table is compacted), popcount prefix
    const u64 total_reads = h->run.n_reads + h->run.extra_reads;
    const u64 words = bitmap_words(total_reads), lines = words / BM_LINE;
    const u64 nnz_max = std::min<u64>(E * INL + arena_used(h), (1ull << 32) - 1);     // every key pair there can be
    u32 *bitmap = nullptr, *wpop = nullptr, *wprefix = nullptr, *ord2_raw = nullptr;
    uint2* list_fn = nullptr;
    u64* d_tot = nullptr;                            // [0] occupied slots, [1] distinct first reads, [2] nnz, [3] long rows (u32)
    POOL(h, P_BITMAP, bitmap, words); POOL(h, P_WPOP, wpop, lines); POOL(h, P_WPREFIX, wprefix, lines);
    POOL(h, P_ROWLEN, ord2_raw, 2 * E); POOL(h, P_LISTFN, list_fn, E);
    uint2* ord2 = reinterpret_cast<uint2*>(ord2_raw);           // (slot, row length) by rank
    POOL(h, P_ORDER, h->run.csr.order, E);
    POOL(h, P_INDPTR, h->run.csr.indptr, E + 1); POOL(h, P_COUNTS, h->run.csr.counts, E);
    POOL(h, P_INDICES, h->run.csr.indices, nnz_max); POOL(h, P_DATA, h->run.csr.data, nnz_max);
    POOL(h, P_TOTALS, d_tot, 8);
    u32* big = nullptr;
    POOL(h, P_MS_X, big, E);
    u32* d_nbig = reinterpret_cast<u32*>(d_tot + 3);
    HIPCHK(h, hipMemsetAsync(bitmap, 0, words * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(d_tot, 0, 8 * sizeof(u64), h->stream));
    bool listed = false;
    if (h->can_push() && h->run.n_reads) {             // the usual case: the counting pass lists the occupied slots as it goes
        u32* list = nullptr;
        POOL(h, P_LIST, list, E);
        const CompactSink sink{list, E, d_tot, bitmap, total_reads, list_fn};
        RCCHK(ensure_counts(h, &sink, &listed));
    } else if (!h->has_result()) {
        RCCHK(ensure_counts(h));
    }
    if (!listed) {                                     // (counts were made earlier -- a table export, a merge -- or there were none to make)
        if (!h->has_result() && h->run.d_list_n)       // ... and the list with them (a merged key range): no scan of the table
            k_list_fn<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->table, h->slot_list(), E, h->run.d_list_n, d_tot, bitmap, total_reads, list_fn);
        else
            RCCHK(compact_table_dev(h, d_tot, bitmap, total_reads, list_fn));
    }
    k_popc<<<nblk(lines, TPB), TPB, 0, h->stream>>>(bitmap, lines, wpop);
    RCCHK(excl_scan_dev(h, wpop, lines, wprefix, d_tot + 1));
    k_rank<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->slot_list(), list_fn, E, total_reads, bitmap, wprefix, ord2);
    RCCHK(excl_scan_dev(h, ord2_raw + 1, E, h->run.csr.indptr, d_tot + 2, 2, h->run.csr.indptr + E));
    k_emit_small<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->table, ord2, h->run.csr.order, E, h->arena, h->run.csr.indptr, h->run.csr.indices, h->run.csr.data,
                                                       h->run.csr.counts, h->cfg.n_loci, h->cfg.n_haplotypes, big, d_nbig, h->ctr);
    // long rows, one wave each: a fixed launch that walks the queue (its length stays on the device)
    k_emit_big<<<(unsigned)std::min<u64>(nblk(E * 64, TPB), 2048), TPB, 0, h->stream>>>(h->table, h->run.csr.order, big, d_nbig, h->arena, h->run.csr.indptr,
                                                                                       h->run.csr.indices, h->run.csr.data, h->cfg.n_loci, h->cfg.n_haplotypes, h->ctr);
    u64* const tot = h->pin_out->tot;
    HIPCHK(h, hipMemcpyAsync(tot, d_tot, 4 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    RCCHK(run_refused(h, sync_counters(h)));           // the one wait (an index out of range that only the emit sees, a count beyond int32: the run cannot end)
    h->run.n_list = tot[0];
    if (tot[0] != E) return fail(h, ECB_ERR_HIP, "internal: %llu occupied slots but %llu ECs created", (unsigned long long)tot[0], (unsigned long long)E);
    if (tot[1] != E) return fail(h, ECB_ERR_HIP, "internal: %llu distinct first-appearance indices for %llu ECs", (unsigned long long)tot[1], (unsigned long long)E);
    RCCHK(refuse_nnz(h, tot[2]));
    h->run.sizes = result_sizes(E, tot[2], h->hctr.all + h->run.extra_all, valid, total_reads);
    if (h->multisample()) {
        if (h->run.origin == Origin::ADOPTED) {                            // multi-GPU: the triples arrive through ecb_ms_adopt_triples_device
            h->run.tri.n = 0; h->run.sizes.n_samples = 0; h->run.sizes.nnz_n = 0;
        } else {
            if (h->run.extra_reads) return fail(h, ECB_ERR_STATE, "multisample across GPUs: adopt the merged ECs (ecb_table_adopt_device), then ecb_ms_adopt_triples_device");
            RCCHK(ensure_slot_ranks(h, E));
            RCCHK(ms_reduce(h, h->run.csr.rank_of_slot));
            h->run.sizes.n_samples = 0; h->run.sizes.nnz_n = h->run.tri.n;
        }
    }
    h->run.stage = Stage::FINAL;
    *out = h->run.sizes;
    return ECB_OK;
}

int ecb_export_firsts_device(ecb_handle* h, void* d_firsts) {
    if (!h || !d_firsts) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_result() || h->run.origin == Origin::ASSEMBLED) return fail(h, ECB_ERR_STATE, "first reads are exported from a finalized table");
    HIPCHK(h, hipSetDevice(h->device));
    const u64 E = h->run.sizes.n_ecs;
    k_export_firsts<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->table, h->run.csr.order, E, (u32*)d_firsts);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_assemble_ranges_device(ecb_handle* h, uint32_t n_pieces, const void* const* d_indptr, const void* const* d_indices,
                               const void* const* d_data, const void* const* d_counts, const void* const* d_firsts,
                               const uint64_t* n_ecs, const uint64_t* nnz, uint64_t total_reads, uint64_t all_alignments,
                               uint64_t valid_alignments, ecb_sizes* out) {
    if (!h || !out) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (h->has_result() || h->run.origin == Origin::ADOPTED || !h->holds_nothing()) return fail(h, ECB_ERR_STATE, "assembling needs an empty handle");
    if (n_pieces && (!d_indptr || !d_indices || !d_data || !d_counts || !d_firsts || !n_ecs || !nnz)) return fail(h, ECB_ERR_ARG, "null piece lists");
    if (n_pieces > 65535u) return fail(h, ECB_ERR_LIMIT, "at most 65535 pieces");
    u64 E = 0, NNZ = 0;
    for (u32 q = 0; q < n_pieces; ++q) {
        if (n_ecs[q] && (!d_indptr[q] || !d_counts[q] || !d_firsts[q] || (nnz[q] && (!d_indices[q] || !d_data[q])))) return fail(h, ECB_ERR_ARG, "null piece buffers");
        E += n_ecs[q]; NNZ += nnz[q];
    }
    RCCHK(refuse_no_ecs(h, E, valid_alignments));
    RCCHK(refuse_nnz(h, NNZ));
    if (total_reads >= (1ull << 32) - 1) return fail(h, ECB_ERR_LIMIT, "more than 2^32-2 reads in total");
    HIPCHK(h, hipSetDevice(h->device));
    h->run.csr = {};
    const u64 words = bitmap_words(total_reads), lines = words / BM_LINE;
    u32 *bitmap = nullptr, *wpop = nullptr, *wprefix = nullptr, *place_raw = nullptr;
    u64* d_tot = nullptr;
    POOL(h, P_BITMAP, bitmap, words); POOL(h, P_WPOP, wpop, lines); POOL(h, P_WPREFIX, wprefix, lines);
    POOL(h, P_ROWLEN, place_raw, 4 * E);
    uint4* place = reinterpret_cast<uint4*>(place_raw);         // {EC within its piece + 1, row length, count, piece} by rank
    POOL(h, P_INDPTR, h->run.csr.indptr, E + 1); POOL(h, P_COUNTS, h->run.csr.counts, E);
    POOL(h, P_INDICES, h->run.csr.indices, std::max<u64>(NNZ, 1)); POOL(h, P_DATA, h->run.csr.data, std::max<u64>(NNZ, 1));
    POOL(h, P_TOTALS, d_tot, 8);
    HIPCHK(h, hipMemsetAsync(bitmap, 0, words * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(d_tot, 0, 8 * sizeof(u64), h->stream));
    HIPCHK(h, hipMemsetAsync(place_raw, 0, E * 16, h->stream));
    RCCHK(clear_counters(h));
    std::vector<PieceDesc> desc;
    u64 most = 0;
    for (u32 q = 0, at = 0; q < n_pieces; ++q) {
        if (!n_ecs[q]) continue;
        desc.push_back(PieceDesc{(const u32*)d_firsts[q], (const int*)d_indptr[q], (const int*)d_indices[q], (const int*)d_data[q], (const int*)d_counts[q],
                                 n_ecs[q], nnz[q], at});
        at += n_ecs[q]; most = std::max<u64>(most, n_ecs[q]);
    }
    u64* d_desc_raw = nullptr;
    POOL(h, P_PARTS, d_desc_raw, desc.size() * sizeof(PieceDesc) / sizeof(u64));
    const PieceDesc* d_desc = reinterpret_cast<const PieceDesc*>(d_desc_raw);
    HIPCHK(h, hipMemcpyAsync(d_desc_raw, desc.data(), desc.size() * sizeof(PieceDesc), hipMemcpyHostToDevice, h->stream));
    const dim3 grid((unsigned)nblk(most, TPB), (unsigned)desc.size());
    k_mark_bits<<<grid, TPB, 0, h->stream>>>(d_desc, total_reads, bitmap, h->ctr);
    k_popc<<<nblk(lines, TPB), TPB, 0, h->stream>>>(bitmap, lines, wpop);
    RCCHK(excl_scan_dev(h, wpop, lines, wprefix, d_tot + 1));
    k_piece_place<<<grid, TPB, 0, h->stream>>>(d_desc, E, total_reads, bitmap, wprefix, place, h->ctr);
    RCCHK(excl_scan_dev(h, place_raw + 1, E, h->run.csr.indptr, d_tot + 2, 4, h->run.csr.indptr + E));
    k_piece_rows<<<nblk(E, TPB), TPB, 0, h->stream>>>(d_desc, (u32)desc.size(), place, E, h->run.csr.indptr, h->run.csr.indices, h->run.csr.data, h->run.csr.counts);
    u64 tot[8];
    HIPCHK(h, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, h->stream));
    h->ctr_synced = false;
    const int rc = sync_counters(h);                         // (waits)
    if (rc == ECB_ERR_CONTRACT) return fail(h, rc, "a piece is malformed: a first read beyond the run's reads, or row offsets that are not its own");
    RCCHK(rc);
    if (tot[1] != E) return fail(h, ECB_ERR_CONTRACT, "the pieces hold %llu ECs but %llu distinct first reads: ranges overlap or a first read is missing",
                                 (unsigned long long)E, (unsigned long long)tot[1]);
    if (tot[2] != NNZ) return fail(h, ECB_ERR_HIP, "internal: %llu non-zeros placed, %llu received", (unsigned long long)tot[2], (unsigned long long)NNZ);
    h->run.sizes = result_sizes(E, NNZ, all_alignments, valid_alignments, total_reads);
    if (h->multisample()) { h->run.sizes.n_samples = 0; h->run.sizes.nnz_n = 0; h->run.tri.n = 0; h->run.triples = Triples::NONE; }   // (N comes with the shards' triples: ecb_ms_adopt_triples_device)
    h->run.stage = Stage::FINAL; h->run.origin = Origin::ASSEMBLED;
    *out = h->run.sizes;
    return ECB_OK;
}

int ecb_export_device(ecb_handle* h, void* ia, void* ja, void* da, void* in_, void* jn, void* dn) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_result()) return fail(h, ECB_ERR_STATE, "export before finalize");
    return export_result(h, ia, ja, da, in_, jn, dn, hipMemcpyDeviceToDevice);
}

int ecb_export(ecb_handle* h, int32_t* ia, int32_t* ja, int32_t* da, int32_t* in_, int32_t* jn, int32_t* dn) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_result()) return fail(h, ECB_ERR_STATE, "export before finalize");
    if (h->multisample() && (in_ || jn || dn))
        return fail(h, ECB_ERR_STATE, "multisample: N comes from ecb_export_pairs");
    return export_result(h, ia, ja, da, in_, jn, dn, hipMemcpyDeviceToHost);
}

int ecb_export_ranges(ecb_handle* h, int64_t* out) {
    if (!h || !out) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!(h->cfg.flags & ECB_F_RANGES)) return fail(h, ECB_ERR_STATE, "handle was created without ECB_F_RANGES");
    HIPCHK(h, hipSetDevice(h->device));
    const u64 ns = (u64)h->cfg.n_loci * h->cfg.n_haplotypes;
    long long* d = nullptr;                            // (the handle's pool: nothing to free on an early return)
    POOL(h, P_EXPORT, d, ns);
    k_range_len<<<nblk(ns, TPB), TPB, 0, h->stream>>>(h->rng, ns, d);
    HIPCHK(h, hipMemcpyAsync(out, d, ns * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_export_range_minmax(ecb_handle* h, int32_t* mn, int32_t* mx) {
    if (!h || !mn || !mx) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!(h->cfg.flags & ECB_F_RANGES)) return fail(h, ECB_ERR_STATE, "handle was created without ECB_F_RANGES");
    HIPCHK(h, hipSetDevice(h->device));
    const u64 ns = (u64)h->cfg.n_loci * h->cfg.n_haplotypes;
    int* d = nullptr;
    POOL(h, P_EXPORT, d, 2 * ns);
    k_split_minmax<<<nblk(ns, TPB), TPB, 0, h->stream>>>(h->rng, ns, d, d + ns);
    HIPCHK(h, hipMemcpyAsync(mn, d, ns * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(mx, d + ns, ns * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_export_pairs(ecb_handle* h, uint32_t* ec, uint32_t* meta, uint32_t* count, uint32_t* first_read) {
    if (!h || !ec || !meta || !count || !first_read) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_ms_result()) return fail(h, ECB_ERR_STATE, "no multisample result");
    HIPCHK(h, hipSetDevice(h->device));
    const u64 nt = h->run.tri.n;
    u32* x = nullptr;
    POOL(h, P_MS_X, x, 3 * nt);
    if (h->awaits_triples()) return fail(h, ECB_ERR_STATE, "multisample across GPUs: no triples adopted yet (ecb_ms_adopt_triples_device)");
    k_ms_split<<<nblk(nt, TPB), TPB, 0, h->stream>>>(h->run.tri.okey, h->run.tri.ostart, h->run.tri.ocount, nt, x, x + nt, x + 2 * nt);
    HIPCHK(h, hipMemcpyAsync(ec, x, nt * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(meta, x + nt, nt * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(count, x + 2 * nt, nt * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(first_read, h->run.tri.ofirst, nt * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_export_read_ec(ecb_handle* h, int32_t* out) {
    if (!h || !out) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_result()) return fail(h, ECB_ERR_STATE, "export before finalize");
    if (h->run.extra_reads || h->run.origin == Origin::ASSEMBLED) return fail(h, ECB_ERR_STATE, "per-read EC ids are not kept across a multi-GPU merge");
    HIPCHK(h, hipSetDevice(h->device));
    int* d = nullptr;
    POOL(h, P_EXPORT, d, h->run.n_reads);
    RCCHK(ensure_slot_ranks(h, h->run.sizes.n_ecs));
    k_read_ec<<<nblk(h->run.n_reads, TPB), TPB, 0, h->stream>>>(h->read_slot, h->run.n_reads, h->run.csr.rank_of_slot, d);
    HIPCHK(h, hipMemcpyAsync(out, d, h->run.n_reads * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_table_sizes(ecb_handle* h, uint64_t* n_entries, uint64_t* n_pairs, uint64_t* n_reads) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (h->open_read()) RCCHK(stage_and_process(h, nullptr, nullptr, nullptr, nullptr, 0));
    RCCHK(sync_counters(h));
    RCCHK(ensure_counts(h));
    if (n_entries) *n_entries = h->n_ecs();
    if (n_pairs) *n_pairs = h->n_ecs() * INL + arena_used(h);      // (an upper bound: up to INL pairs per EC sit in its slot)
    if (n_reads) *n_reads = h->run.n_reads;
    return ECB_OK;
}

int ecb_table_export_device(ecb_handle* h, void* d_entries, void* d_pairs, uint64_t read_base) {
    uint64_t eo[2], po[2];                             // one part: entries in table order, their keys packed behind each other
    return ecb_table_export_parts_device(h, d_entries, d_pairs, read_base, 1, eo, po);
}

int ecb_table_merge_batch_device(ecb_handle* h, uint32_t n_tables, const void* const* d_entries, const uint64_t* n_entries,
                                const void* const* d_pairs, const uint64_t* n_pairs) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (h->has_result()) return fail(h, ECB_ERR_STATE, "merge after finalize");
    if (h->run.origin == Origin::ADOPTED) return fail(h, ECB_ERR_STATE, "merge into a table that adopted entries");
    if (n_tables && (!d_entries || !n_entries || !d_pairs || !n_pairs)) return fail(h, ECB_ERR_ARG, "null table lists");
    u64 total = 0;
    for (u32 t = 0; t < n_tables; ++t) {
        if (n_entries[t] && (!d_entries[t] || (n_pairs[t] && !d_pairs[t]))) return fail(h, ECB_ERR_ARG, "null table buffers");
        total += n_entries[t];
    }
    if (!total) return ECB_OK;
    HIPCHK(h, hipSetDevice(h->device));
    RCCHK(sync_counters(h));
    RCCHK(ensure_counts(h));                       // own reads first: merged counts are added on top
    // room for every entry being new: one growth up front, then the merges queue up behind each other with one sync at the end
    while ((h->n_ecs() + total) * 2 > h->cap) { RCCHK(grow_table(h, h->cap * 4)); }
    HIPCHK(h, hipMemsetAsync(&h->ctr->n_queue, 0, sizeof(u64), h->stream));
    // New ECs may join.  The list of occupied slots is carried along when it can be: the table is empty (the handle that merges one
    // key range), or its list is current and has room (a buffer that had to grow would lose what it holds).
    u32* mlist = nullptr;
    const u64 list_need = h->n_ecs() + total;
    if (h->n_ecs() == 0 || (h->run.d_list_n && h->pool[ecb_handle::P_LIST].bytes >= list_need * sizeof(u32))) {
        const bool fresh = h->n_ecs() == 0;
        POOL(h, P_LIST, mlist, list_need);
        if (fresh) { POOL(h, P_CNT, h->run.d_list_n, 1); HIPCHK(h, hipMemsetAsync(h->run.d_list_n, 0, sizeof(u64), h->stream)); }
    } else
        h->run.d_list_n = nullptr;
    std::vector<MergeDesc> desc;
    u64 most = 0;
    for (u32 t = 0; t < n_tables; ++t)
        if (n_entries[t]) { desc.push_back(MergeDesc{(const Entry*)d_entries[t], (const uint2*)d_pairs[t], n_entries[t], n_pairs[t]}); most = std::max<u64>(most, n_entries[t]); }
    if (desc.size() > 65535u) return fail(h, ECB_ERR_LIMIT, "at most 65535 tables per call");
    u64* d_desc = nullptr;
    POOL(h, P_PARTS, d_desc, desc.size() * sizeof(MergeDesc) / sizeof(u64));
    HIPCHK(h, hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(MergeDesc), hipMemcpyHostToDevice, h->stream));
    k_merge<<<dim3((unsigned)nblk(most, MERGE_PER_BLOCK), (unsigned)desc.size()), TPB, 0, h->stream>>>(reinterpret_cast<const MergeDesc*>(d_desc), h->table, h->cap - 1,
                                                                                                        h->arena, h->arena_cap, h->ctr,
                                                                                                        mlist, list_need, h->run.d_list_n);
    RCCHK(run_refused(h, sync_counters(h)));
    if (h->hctr.n_queue) return run_refused(h, fail(h, ECB_ERR_TABLE_FULL, "internal: merge found no slot in a half-empty table"));
    return ECB_OK;
}

int ecb_table_rebase_device(ecb_handle* h, void* d_entries, uint64_t n_entries, uint64_t read_base) {
    if (!h || (n_entries && !d_entries)) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (read_base >= (1ull << 32) - 1) return fail(h, ECB_ERR_LIMIT, "more than 2^32-2 reads in total");
    if (!n_entries || !read_base) return ECB_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // (no wait: ordered on the handle's stream, ahead of a merge or adopt on this handle; an entry that would pass the limit is
    //  reported by the next call that reads the device counters, as ECB_ERR_CONTRACT)
    k_rebase<<<nblk(n_entries, TPB), TPB, 0, h->stream>>>((Entry*)d_entries, n_entries, (u32)read_base, (u32)((1ull << 32) - 1 - read_base), h->ctr);
    h->ctr_synced = false;
    return ECB_OK;
}

int ecb_table_merge_device(ecb_handle* h, const void* d_entries, uint64_t n_entries, const void* d_pairs, uint64_t n_pairs) {
    return ecb_table_merge_batch_device(h, 1, &d_entries, &n_entries, &d_pairs, &n_pairs);
}

int ecb_table_export_parts_device(ecb_handle* h, void* d_entries, void* d_pairs, uint64_t read_base, uint32_t n_parts,
                                  uint64_t* entry_offsets, uint64_t* pair_offsets) {
    if (!h || !d_entries || !d_pairs || !entry_offsets || !pair_offsets) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (n_parts == 0 || n_parts > MAX_PARTS) return fail(h, ECB_ERR_LIMIT, "1 .. %u parts", MAX_PARTS);
    HIPCHK(h, hipSetDevice(h->device));
    RCCHK(sync_counters(h));
    if (read_base + h->run.n_reads >= (1ull << 32) - 1) return fail(h, ECB_ERR_LIMIT, "more than 2^32-2 reads in total");
    RCCHK(ensure_counts(h));
    RCCHK(compact_table(h));
    const u64 E = h->n_ecs();
    u64* d_cnt = nullptr;                              // [0, 2P): counts, then cursors; [2P, 3P): first pair of every part
    POOL(h, P_PARTS, d_cnt, 3 * (u64)n_parts);
    HIPCHK(h, hipMemsetAsync(d_cnt, 0, 2 * n_parts * sizeof(u64), h->stream));
    if (E) k_parts_count<<<nblk(E, PARTS_PER_BLOCK), TPB, 0, h->stream>>>(h->table, h->slot_list(), E, n_parts, d_cnt);
    std::vector<u64> cnt(2 * n_parts), cur(3 * n_parts);
    HIPCHK(h, hipMemcpyAsync(cnt.data(), d_cnt, 2 * n_parts * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    entry_offsets[0] = pair_offsets[0] = 0;
    for (u32 q = 0; q < n_parts; ++q) {
        entry_offsets[q + 1] = entry_offsets[q] + cnt[q];
        pair_offsets[q + 1] = pair_offsets[q] + cnt[n_parts + q];
        cur[q] = entry_offsets[q]; cur[n_parts + q] = pair_offsets[q]; cur[2 * n_parts + q] = pair_offsets[q];
    }
    HIPCHK(h, hipMemcpyAsync(d_cnt, cur.data(), 3 * n_parts * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    if (E) {
        u64* big = nullptr;                            // long keys: (first pair, slot << 32 | length) + their number behind the list
        POOL(h, P_BIG, big, 2 * E + 1);
        u32* d_nbig = reinterpret_cast<u32*>(big + 2 * E);
        HIPCHK(h, hipMemsetAsync(d_nbig, 0, sizeof(u64), h->stream));
        k_parts_export<<<nblk(E, PARTS_PER_BLOCK), TPB, 0, h->stream>>>(h->table, h->slot_list(), E, h->arena, n_parts, d_cnt, d_cnt + 2 * n_parts,
                                                                   (Entry*)d_entries, (uint2*)d_pairs, (u32)read_base, big, d_nbig);
        u32 n_big = 0;
        HIPCHK(h, hipMemcpyAsync(&n_big, d_nbig, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));      // (cur lives on this stack frame)
        if (n_big) k_parts_sort_big<<<nblk((u64)n_big * 64, TPB), TPB, 0, h->stream>>>(h->table, h->arena, big, n_big, (uint2*)d_pairs);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_table_adopt_batch_device(ecb_handle* h, uint32_t n_tables, const void* const* d_entries, const uint64_t* n_entries,
                                const void* const* d_pairs, const uint64_t* n_pairs) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (h->has_result()) return fail(h, ECB_ERR_STATE, "adopt after finalize");
    if (n_tables && (!d_entries || !n_entries || !d_pairs || !n_pairs)) return fail(h, ECB_ERR_ARG, "null table lists");
    HIPCHK(h, hipSetDevice(h->device));
    RCCHK(sync_counters(h));
    if (h->run.origin != Origin::ADOPTED && !h->holds_nothing())
        return fail(h, ECB_ERR_STATE, "adopt needs an empty handle (use ecb_table_merge_device to add to a built table)");
    u64 add_e = 0, add_p = 0;
    for (u32 t = 0; t < n_tables; ++t) {
        if (n_entries[t] && (!d_entries[t] || (n_pairs[t] && !d_pairs[t]))) return fail(h, ECB_ERR_ARG, "null table buffers");
        if (n_entries[t]) { add_e += n_entries[t]; add_p += n_pairs[t]; }
    }
    h->run.origin = Origin::ADOPTED; h->run.stage = Stage::COUNTED; h->run.d_list_n = nullptr;
    if (!add_e) return ECB_OK;
    u64 have = h->n_ecs(), top = h->hctr.arena_top;
    if (top + add_p > h->arena_cap || top + add_p >= (1ull << 32))      // (nothing was copied, but the handle is an adopting one by now and cannot take this table)
        return run_refused(h, fail(h, ECB_ERR_TABLE_FULL, "EC key arena exhausted (%llu pairs): raise arena_capacity", (unsigned long long)h->arena_cap));
    if (have + add_e > h->cap) {                        // consecutive slots: a bigger array and a copy, no rehash
        u64 nc = h->cap;
        while (nc < have + add_e) nc *= 2;
        HIPCHK(h, h->table.grow(nc * sizeof(Slot), 0, have * sizeof(Slot), h->stream));
        h->cap = nc;
    }
    for (u32 t = 0; t < n_tables; ++t) {
        if (!n_entries[t]) continue;
        k_adopt<<<nblk(n_entries[t], TPB), TPB, 0, h->stream>>>((const Entry*)d_entries[t], n_entries[t], (const uint2*)d_pairs[t], h->table, have, (u32)top);
        if (n_pairs[t]) HIPCHK(h, hipMemcpyAsync(h->arena + top, d_pairs[t], n_pairs[t] * sizeof(uint2), hipMemcpyDeviceToDevice, h->stream));
        have += n_entries[t]; top += n_pairs[t];
    }
    h->hctr.n_ecs = have; h->hctr.arena_top = top;
    HIPCHK(h, hipMemcpyAsync(&h->ctr->n_ecs, &h->hctr.n_ecs, sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(&h->ctr->arena_top, &h->hctr.arena_top, sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_table_adopt_device(ecb_handle* h, const void* d_entries, uint64_t n_entries, const void* d_pairs, uint64_t n_pairs) {
    return ecb_table_adopt_batch_device(h, 1, &d_entries, &n_entries, &d_pairs, &n_pairs);
}

int ecb_export_ec_keys_device(ecb_handle* h, void* d_keys) {
    if (!h || !d_keys) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_result()) return fail(h, ECB_ERR_STATE, "export before finalize");
    HIPCHK(h, hipSetDevice(h->device));
    const u64 E = h->run.sizes.n_ecs;
    if (h->run.origin == Origin::ASSEMBLED) k_row_keys<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->run.csr.indptr, h->run.csr.indices, h->run.csr.data, E, (u64*)d_keys);     // (no table behind an assembled result)
    else k_export_keys<<<nblk(E, TPB), TPB, 0, h->stream>>>(h->table, h->run.csr.order, E, (u64*)d_keys);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_ms_local_triples_device(ecb_handle* h, const void* d_keys, const void* d_indptr_a, const void* d_indices_a, const void* d_data_a,
                                uint64_t n_ecs, uint64_t read_base, void* d_key, void* d_count, void* d_first, uint64_t* n_triples) {
    if (!h || !n_triples) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->multisample()) return fail(h, ECB_ERR_STATE, "handle was created without ECB_F_MULTISAMPLE");
    if (h->has_result() || h->run.origin == Origin::ADOPTED) return fail(h, ECB_ERR_STATE, "a shard's triples come from the handle its reads were pushed into");
    *n_triples = 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->open_read()) RCCHK(stage_and_process(h, nullptr, nullptr, nullptr, nullptr, 0));   // the stream ends here: the carried read is complete
    if (!h->run.n_reads) return ECB_OK;
    if (!d_keys || !d_indptr_a || !d_indices_a || !d_data_a || !d_key || !d_count || !d_first) return fail(h, ECB_ERR_ARG, "null buffers");
    if (read_base + h->run.n_reads >= (1ull << 32) - 1) return fail(h, ECB_ERR_LIMIT, "more than 2^32-2 reads in total");
    HIPCHK(h, hipSetDevice(h->device));
    RCCHK(sync_counters(h));
    u32* grank = nullptr;
    POOL(h, P_MS_GRANK, grank, h->cap);
    HIPCHK(h, hipMemsetAsync(grank, 0xFF, h->cap * sizeof(u32), h->stream));
    k_set_global_rank<<<nblk(n_ecs, TPB), TPB, 0, h->stream>>>((const u64*)d_keys, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                                                              n_ecs, h->table, h->cap - 1, h->arena, grank);
    RCCHK(ms_reduce(h, grank));
    const u64 nt = h->run.tri.n;
    u64 last = 0;                                     // keys are sorted: an EC id of 0xFFFFFFFF would be the last one
    HIPCHK(h, hipMemcpyAsync(&last, h->run.tri.okey + (nt - 1), sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((last >> 32) == 0xFFFFFFFFull) return fail(h, ECB_ERR_CONTRACT, "a read's EC is missing from the merged EC list");
    k_ms_out<<<nblk(nt, TPB), TPB, 0, h->stream>>>(h->run.tri.okey, h->run.tri.ofirst, h->run.tri.ostart, nt, (u32)read_base, (u64*)d_key, (u32*)d_count, (u32*)d_first);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_triples = nt;
    return ECB_OK;
}

int ecb_ms_adopt_triples_device(ecb_handle* h, uint32_t n_tables, const void* const* d_key, const void* const* d_count,
                                const void* const* d_first, const uint64_t* n, uint64_t* n_triples) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->multisample()) return fail(h, ECB_ERR_STATE, "handle was created without ECB_F_MULTISAMPLE");
    if (!h->has_result() || !h->entries_from_elsewhere()) return fail(h, ECB_ERR_STATE, "triples are adopted by the finalized handle that adopted the merged ECs (or assembled their ranges)");
    if (n_tables && (!d_key || !d_count || !d_first || !n)) return fail(h, ECB_ERR_ARG, "null lists");
    HIPCHK(h, hipSetDevice(h->device));
    u64 tot = 0;
    for (u32 t = 0; t < n_tables; ++t) { if (n[t] && (!d_key[t] || !d_count[t] || !d_first[t])) return fail(h, ECB_ERR_ARG, "null buffers"); tot += n[t]; }
    if (tot >= (1ull << 32)) return fail(h, ECB_ERR_LIMIT, "more than 2^32-1 triples");
    u64 *keys = nullptr, *keys2 = nullptr; u32 *vals = nullptr, *vals2 = nullptr, *flag = nullptr, *pos = nullptr, *cin = nullptr, *fin = nullptr;
    POOL(h, P_MS_KEYS, keys, tot); POOL(h, P_MS_KEYS2, keys2, tot); POOL(h, P_MS_VALS, vals, tot); POOL(h, P_MS_VALS2, vals2, tot);
    POOL(h, P_MS_FLAG, flag, tot); POOL(h, P_MS_POS, pos, tot); POOL(h, P_MS_CIN, cin, tot); POOL(h, P_MS_FIN, fin, tot);
    u64 at = 0;
    for (u32 t = 0; t < n_tables; ++t) {
        if (!n[t]) continue;
        HIPCHK(h, hipMemcpyAsync(keys + at, d_key[t], n[t] * 8, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(cin + at, d_count[t], n[t] * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(fin + at, d_first[t], n[t] * 4, hipMemcpyDeviceToDevice, h->stream));
        at += n[t];
    }
    u64 nt = 0;
    if (tot) {
        k_ms_swz_keys<<<nblk(tot, TPB), TPB, 0, h->stream>>>(keys, tot);      // (sorted as (EC, cell, file), like a handle's own triples)
        k_iota<<<nblk(tot, TPB), TPB, 0, h->stream>>>(vals, tot);
        SortBufs s{{keys, keys2}, {vals, vals2}};
        RCCHK(sorted_runs(h, s, tot, flag, pos, &nt));
        POOL(h, P_MS_OKEY, h->run.tri.okey, nt); POOL(h, P_MS_OFIRST, h->run.tri.ofirst, nt); POOL(h, P_MS_OCOUNT, h->run.tri.ocount, nt);
        HIPCHK(h, hipMemsetAsync(h->run.tri.ocount, 0, (u64)nt * 4, h->stream));
        HIPCHK(h, hipMemsetAsync(h->run.tri.ofirst, 0xFF, (u64)nt * 4, h->stream));
        k_ms_combine<<<nblk(tot, TPB), TPB, 0, h->stream>>>(s.keys(), s.vals(), flag, pos, tot, cin, fin, h->run.tri.okey, h->run.tri.ocount, h->run.tri.ofirst);
        u64 last = 0;
        HIPCHK(h, hipMemcpyAsync(&last, s.keys() + (tot - 1), sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((last >> 32) >= h->run.sizes.n_ecs) return fail(h, ECB_ERR_CONTRACT, "triple with an EC id beyond the merged ECs");
    }
    h->run.tri.n = nt; h->run.triples = Triples::ADOPTED;
    h->run.sizes.n_samples = 0; h->run.sizes.nnz_n = nt;
    if (n_triples) *n_triples = nt;
    return ECB_OK;
}

int ecb_ms_filter(ecb_handle* h, uint32_t n_cells, int64_t minimum_count, ecb_ms_sizes* out) {
    if (!h || !out) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->has_ms_result()) return fail(h, ECB_ERR_STATE, "no multisample result");
    if (h->awaits_triples()) return fail(h, ECB_ERR_STATE, "multisample across GPUs: no triples adopted yet (ecb_ms_adopt_triples_device)");
    if (!n_cells || n_cells > (1u << ECB_CELL_BITS)) return fail(h, ECB_ERR_ARG, "n_cells out of range");
    HIPCHK(h, hipSetDevice(h->device));
    h->run.flt = {};                                 // (until this call succeeds: its pool buffers are regrown under the last result)
    ecb_handle::Run::Filtered f;
    hipStream_t st = h->stream;
    const u64 T = h->run.tri.n, E = h->run.sizes.n_ecs;
    const u64 min_count = minimum_count <= 0 ? 1ull : (u64)minimum_count;          // bam_utils_multisample.py:596-597
    if (!T) return fail(h, ECB_ERR_EMPTY, "no (EC, cell) counts: nothing to filter");
    // The triples are sorted by (EC, cell, file) (ms_reduce / ecb_ms_adopt_triples_device).  Everything read-sized below is a
    // linear pass over them; the only sort left is the one that turns the surviving (EC, cell) pairs -- in EC order -- into
    // the columns of N, on the digits of the cell alone.  The triple-sized buffers are the ones ms_reduce sorted in (its pool).
    u32 *x = nullptr, *flag = nullptr, *pos = nullptr, *v0 = nullptr, *v1 = nullptr;
    u64 *k0 = nullptr, *k1 = nullptr;
    POOL(h, P_MS_TMP, x, 3 * T);
    POOL(h, P_MS_FLAG, flag, std::max<u64>(T, n_cells)); POOL(h, P_MS_POS, pos, std::max<u64>(T, n_cells));
    POOL(h, P_MS_KEYS, k0, T); POOL(h, P_MS_KEYS2, k1, T); POOL(h, P_MS_VALS, v0, T); POOL(h, P_MS_VALS2, v1, T);
    u32 *ec = x, *meta = x + T, *cnt = x + 2 * T;
    k_ms_split<<<nblk(T, TPB), TPB, 0, st>>>(h->run.tri.okey, h->run.tri.ostart, h->run.tri.ocount, T, ec, meta, cnt);
    const u32* first = h->run.tri.ofirst;
    std::vector<DevBuf<>> sc;                                              // (cell- and EC-sized scratch: small)
    u64 *total = fresh<u64>(sc, n_cells), *cellkey = fresh<u64>(sc, n_cells);
    u32 *firstfile = fresh<u32>(sc, n_cells), *seg = fresh<u32>(sc, E + 1), *keep_ec = fresh<u32>(sc, E), *new_rank = fresh<u32>(sc, E), *new_cell = fresh<u32>(sc, n_cells);
    u32* d_err = fresh<u32>(sc, 1);
    if (missing(sc)) return fail(h, ECB_ERR_HIP, "out of device memory");
    HIPCHK(h, hipMemsetAsync(total, 0, (u64)n_cells * 8, st));
    HIPCHK(h, hipMemsetAsync(cellkey, 0xFF, (u64)n_cells * 8, st));
    HIPCHK(h, hipMemsetAsync(firstfile, 0xFF, (u64)n_cells * 4, st));
    HIPCHK(h, hipMemsetAsync(keep_ec, 0, E * 4, st));
    HIPCHK(h, hipMemsetAsync(d_err, 0, 4, st));
    // 1. per cell: reads and first file
    {
        const bool lds = n_cells <= MSF_LDS_CELLS;
        const unsigned grid = (unsigned)std::min<u64>(lds ? 512 : 2048, nblk(T, TPB_MSF));
        k_msf2_cells<<<grid, TPB_MSF, lds ? (size_t)n_cells * 8 : 0, st>>>(meta, cnt, T, n_cells, total, firstfile, d_err);
    }
    // 2. per EC: its first appearance in every file; where every cell enters the cell order; whether the EC keeps a cell
    k_msf2_seg<<<nblk(T, TPB), TPB, 0, st>>>(ec, T, (u32)E, seg, d_err);
    {
        u32* big = fresh<u32>(sc, E + 1);                       // ECs of more than MSF_SMALL triples, their number behind the list
        const u64 max_giant = T / MSF_GIANT + 1;             // ... and of more than MSF_GIANT, with their per-file first appearances
        u32 *giant = fresh<u32>(sc, max_giant + 1), *gfec = fresh<u32>(sc, max_giant * MSF_FILES);
        if (missing(sc)) return fail(h, ECB_ERR_HIP, "out of device memory");
        HIPCHK(h, hipMemsetAsync(big + E, 0, 4, st));
        HIPCHK(h, hipMemsetAsync(giant + max_giant, 0, 4, st));
        HIPCHK(h, hipMemsetAsync(gfec, 0xFF, max_giant * MSF_FILES * 4, st));
        k_msf2_ecs_small<<<nblk(E, TPB), TPB, 0, st>>>(meta, first, seg, (u32)E, n_cells, total, firstfile, min_count, cellkey, keep_ec, big, big + E, giant, giant + max_giant);
        k_msf2_ecs_big<<<(unsigned)std::min<u64>(std::max<u64>(E / MSF_SMALL, 1), 4096), TPB, 0, st>>>(meta, first, seg, big, big + E, n_cells, total, firstfile, min_count, cellkey, keep_ec);
        k_msf2_giant_fec<<<1024, TPB, 0, st>>>(meta, first, seg, giant, giant + max_giant, n_cells, total, min_count, gfec, keep_ec);
        k_msf2_giant_offer<<<1024, TPB, 0, st>>>(meta, first, seg, giant, giant + max_giant, n_cells, firstfile, gfec, cellkey);
    }
    // 3. cell order: by (first appearance of the EC in the cell's first file, first read), then -- stable -- by that file
    k_msf2_cellflag<<<nblk(n_cells, TPB), TPB, 0, st>>>(total, n_cells, flag);
    u64 C = 0;
    RCCHK(excl_scan(h, flag, n_cells, pos, &C));
    // (the bits come in the table's order: 1 and 2 from the passes above, 4 from k_msf2_pairs below, behind this check)
    static const ErrBit MSF_ERRS[] = {
        {1u, ECB_ERR_CONTRACT, "triple with an EC id beyond the finalized ECs"},
        {2u, ECB_ERR_CONTRACT, "a read's cell id is not below n_cells"},
        {4u, ECB_ERR_LIMIT, "an entry of N (the reads of one EC in one cell) is above 2^31-1"},
    };
    u32 err = 0;
    HIPCHK(h, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    RCCHK(refuse_bits(h, MSF_ERRS, err));
    if (!C) return fail(h, ECB_ERR_EMPTY, "no (EC, cell) counts: nothing to filter");
    u32 *cell_id = fresh<u32>(sc, C), *corder = fresh<u32>(sc, C), *corder2 = fresh<u32>(sc, C), *cflag = fresh<u32>(sc, C), *cpos = fresh<u32>(sc, C);
    u64 *ctotal = fresh<u64>(sc, C), *bhi = fresh<u64>(sc, C), *blo = fresh<u64>(sc, C), *ck0 = fresh<u64>(sc, C), *ck1 = fresh<u64>(sc, C);
    if (missing(sc)) return fail(h, ECB_ERR_HIP, "out of device memory");
    k_msf2_celllist<<<nblk(n_cells, TPB), TPB, 0, st>>>(total, firstfile, cellkey, flag, pos, n_cells, cell_id, ctotal, bhi, blo);
    k_iota<<<nblk(C, TPB), TPB, 0, st>>>(corder, C);
    HIPCHK(h, hipMemcpyAsync(ck0, blo, C * 8, hipMemcpyDeviceToDevice, st));
    u32* ord = nullptr;
    { SortBufs s{{ck0, ck1}, {corder, corder2}}; RCCHK(handle_sort(h, s, C));
      k_msf_gather64<<<nblk(C, TPB), TPB, 0, st>>>(bhi, s.vals(), C, s.spare_keys());   // (the second key, in the first sort's order)
      SortBufs s2{{s.spare_keys(), s.keys()}, {s.vals(), s.spare_vals()}}; RCCHK(handle_sort(h, s2, C));
      ord = s2.vals(); }
    k_msf_keepflag<<<nblk(C, TPB), TPB, 0, st>>>(ord, ctotal, C, min_count, cflag);
    u64 S = 0;
    RCCHK(excl_scan(h, cflag, C, cpos, &S));
    if (!S) return fail(h, ECB_ERR_EMPTY, "no cell reaches the minimum count");
    POOL(h, P_F_CELLS, f.cells, S);
    HIPCHK(h, hipMemsetAsync(new_cell, 0xFF, (u64)n_cells * 4, st));
    k_msf_newcell<<<nblk(C, TPB), TPB, 0, st>>>(ord, cflag, cpos, cell_id, C, new_cell, f.cells);
    // 4. ECs that keep a cell, re-ranked (bam_utils_multisample.py:611-636)
    u64 E2 = 0, K = 0;
    RCCHK(excl_scan(h, keep_ec, E, new_rank, &E2));
    // 5. N as CSC over (kept EC, kept cell): the surviving (EC, cell) pairs, the reads of their files added up (:737-791), come
    //    in EC order; a stable sort on the cell's digits makes them the columns
    k_msf2_pairflag<<<nblk(T, TPB), TPB, 0, st>>>(ec, meta, T, new_cell, flag);
    RCCHK(excl_scan(h, flag, T, pos, &K));
    if (K >= (1ull << 31)) return fail(h, ECB_ERR_LIMIT, "N has more than 2^31-1 non-zeros");
    k_msf2_pairs<<<nblk(T, TPB), TPB, 0, st>>>(ec, meta, cnt, flag, pos, T, new_cell, new_rank, k0, v0, d_err);
    const u64 nnz_n = K;
    {
        SortBufs s{{k0, k1}, {v0, v1}};
        RCCHK(handle_sort(h, s, K, msb_mask(S - 1) << 32));
        POOL(h, P_F_IPN, f.ipn, S + 1); POOL(h, P_F_IXN, f.ixn, nnz_n); POOL(h, P_F_DAN, f.dan, nnz_n);
        k_split_out<<<nblk(K, TPB), TPB, 0, st>>>(s.keys(), s.vals(), K, f.ixn, f.dan);
        k_row_ptr<<<nblk(S + 1, TPB), TPB, 0, st>>>(s.keys(), K, (u32)S, f.ipn);
    }
    // 6. the rows of A of the ECs that are left
    u32* rowlen2 = fresh<u32>(sc, E2 + 1);
    if (missing(sc)) return fail(h, ECB_ERR_HIP, "out of device memory");
    POOL(h, P_F_IPA, f.ipa, E2 + 1);
    k_msf_rowlen<<<nblk(E, TPB), TPB, 0, st>>>(h->run.csr.indptr, keep_ec, new_rank, E, rowlen2);
    u64 nnz_a = 0;
    RCCHK(excl_scan(h, rowlen2, E2, reinterpret_cast<u32*>(f.ipa), &nnz_a));
    { const u32 last = (u32)nnz_a; HIPCHK(h, hipMemcpyAsync(f.ipa + E2, &last, 4, hipMemcpyHostToDevice, st)); HIPCHK(h, hipStreamSynchronize(st)); }
    POOL(h, P_F_IXA, f.ixa, nnz_a); POOL(h, P_F_DAA, f.daa, nnz_a);
    k_msf_rows<<<nblk(E, TPB), TPB, 0, st>>>(h->run.csr.indptr, h->run.csr.indices, h->run.csr.data, keep_ec, new_rank, reinterpret_cast<const u32*>(f.ipa), E, f.ixa, f.daa);
    HIPCHK(h, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    RCCHK(refuse_bits(h, MSF_ERRS, err));
    h->run.msf.n_cells_seen = C; h->run.msf.n_cells_kept = S; h->run.msf.n_ecs_kept = E2; h->run.msf.nnz_a = nnz_a; h->run.msf.nnz_n = nnz_n;
    h->run.flt = f;
    *out = h->run.msf;
    return ECB_OK;
}

int ecb_ms_export(ecb_handle* h, uint32_t* kept_cells, int32_t* ia, int32_t* ja, int32_t* da, int32_t* in_, int32_t* jn, int32_t* dn) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    if (!h->run.flt.cells) return fail(h, ECB_ERR_STATE, "ecb_ms_export before ecb_ms_filter");
    HIPCHK(h, hipSetDevice(h->device));
    const ecb_ms_sizes& m = h->run.msf;
    const ecb_handle::Run::Filtered& f = h->run.flt;
    if (kept_cells) HIPCHK(h, hipMemcpyAsync(kept_cells, f.cells, m.n_cells_kept * 4, hipMemcpyDeviceToHost, h->stream));
    if (ia) HIPCHK(h, hipMemcpyAsync(ia, f.ipa, (m.n_ecs_kept + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    if (ja) HIPCHK(h, hipMemcpyAsync(ja, f.ixa, m.nnz_a * 4, hipMemcpyDeviceToHost, h->stream));
    if (da) HIPCHK(h, hipMemcpyAsync(da, f.daa, m.nnz_a * 4, hipMemcpyDeviceToHost, h->stream));
    if (in_) HIPCHK(h, hipMemcpyAsync(in_, f.ipn, (m.n_cells_kept + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    if (jn) HIPCHK(h, hipMemcpyAsync(jn, f.ixn, m.nnz_n * 4, hipMemcpyDeviceToHost, h->stream));
    if (dn) HIPCHK(h, hipMemcpyAsync(dn, f.dan, m.nnz_n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ECB_OK;
}

int ecb_counters(ecb_handle* h, uint64_t* all_alignments, uint64_t* valid_alignments, uint64_t* n_reads) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->has_result() && h->open_read()) RCCHK(stage_and_process(h, nullptr, nullptr, nullptr, nullptr, 0));
    RCCHK(sync_counters(h));
    if (all_alignments) *all_alignments = h->hctr.all + h->run.extra_all;
    if (valid_alignments) *valid_alignments = h->hctr.valid + h->run.extra_valid;
    if (n_reads) *n_reads = h->run.n_reads + h->run.extra_reads;
    return ECB_OK;
}

int ecb_add_counters(ecb_handle* h, uint64_t all_alignments, uint64_t valid_alignments, uint64_t n_reads) {
    if (!h) return ECB_ERR_ARG;
    RCCHK(refused_run(h));
    h->run.extra_all += all_alignments; h->run.extra_valid += valid_alignments; h->run.extra_reads += n_reads;
    return ECB_OK;
}

int ecb_profile(ecb_handle* h, int enable) {
    if (!h) return ECB_ERR_ARG;
    h->prof = enable != 0; h->prof_ms = 0; h->prof_launches = 0; h->prof_records = 0;
    return ECB_OK;
}

int ecb_profile_read(ecb_handle* h, double* ms, uint64_t* launches, uint64_t* records) {
    if (!h) return ECB_ERR_ARG;
    if (ms) *ms = h->prof_ms;
    if (launches) *launches = h->prof_launches;
    if (records) *records = h->prof_records;
    return ECB_OK;
}

// the stream kernel the last batch launched, as rocprofv3 names it (k_stream.inc is compiled more than once: which compilation a
// batch takes is decided per batch, in pick_variant)
const char* ecb_profile_kernel(const ecb_handle* h) { return h && h->last_variant != SV_N ? STREAM_VARIANTS[h->last_variant].name : ""; }
#ifdef ECB_TIMING
// profiling build only: the device-wide race counters of k_slow and k_merge (g_race) since the last call, which it zeroes -> 0, or a HIP error
int ecb_timing_race(int device, unsigned long long out[4]) {
    static const u64 zero[4] = {0, 0, 0, 0};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_race), sizeof(zero));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_race), zero, sizeof(zero));
    return (int)e;
}
#endif

}  // extern "C"

// ---- the entry points that take a device instead of a handle (the f-2 conversions, apply-mask, combine, salmon) --------------------------
// Each is one Call.  Its scratch has two backings behind one get: the conversions and apply-mask take theirs from a pool
// kept per device between calls (grown on demand; ecb_release_scratch frees it) -- a config-3-sized conversion needs ~0.4 GB in a dozen
// buffers, and a dozen hipMallocs cost more than its kernels do; combine, salmon and the conversion's sort-everything path take buffers of
// their own, freed with the Call.  The pool serves all threads: g_cv_lock is held from a call's first pool buffer to its end.
namespace {
enum { CV_KEYS0, CV_KEYS1, CV_VALS0, CV_VALS1, CV_HIST, CV_OFFS, CV_SUMS2, CV_BLK, CV_SCAN, CV_HEAD, CV_WORDS, CV_X0, CV_X1, CV_X2, CV_X3, CV_N };
constexpr int CV_MAX_DEV = 64;
DevBuf<>* const g_cv = new DevBuf<>[CV_MAX_DEV * CV_N];      // (never destroyed: no HIP call may run after the runtime has gone, at exit)
std::mutex g_cv_lock;
struct StreamGuard { hipStream_t s = nullptr; ~StreamGuard() { if (s) { hipStreamSynchronize(s); hipStreamDestroy(s); } } };

#define CALLCHK(c, call) HIPCHK_AS(nullptr, (c).prefix, call)
struct Call {
    const int device;
    const char* const prefix;            // of this entry point's ECB_ERR_HIP texts ("combine: ")
    StreamGuard own;                     // the stream of a call that has one of its own (waited for and destroyed after the scratch has gone)
    hipStream_t st = nullptr;            // where the call's work goes: the null stream, or own.s
    std::unique_lock<std::mutex> pool;   // g_cv_lock, once a pool buffer has been handed out
    std::vector<DevBuf<>> keep;          // this call's own buffers
    bool short_of = false;               // a get came back empty
    const int rc;                        // ECB_OK, or why there is no call: the entry point returns it

    Call(int device_, const char* prefix_, bool own_stream = false) : device(device_), prefix(prefix_), rc(open(own_stream)) {}
    // ECB_POISON_SCRATCH: a call that took a pool buffer leaves the device's whole pool filled -- between calls all of it is dead -- once its
    // own work has finished and while it still holds g_cv_lock (the members go after this body: pool among them)
    ~Call() {
        if (!pool || !poison_scratch()) return;
        hipSetDevice(device);
        hipStreamSynchronize(st);
        for (int i = 0; i < CV_N; ++i)
            if (const DevBuf<>& b = g_cv[device * CV_N + i]; b.p) hipMemset(b.p, POISON_BYTE, b.bytes);
        hipDeviceSynchronize();
    }
    int open(bool own_stream) {
        if (device < 0 || device >= CV_MAX_DEV || hipSetDevice(device) != hipSuccess) return fail(nullptr, ECB_ERR_NO_DEVICE, "no such device");
        if (own_stream) { CALLCHK(*this, hipStreamCreate(&own.s)); st = own.s; }
        return ECB_OK;
    }
    // max(n, 1) T's: a fresh buffer that lives as long as the call, or the device's pool buffer `id`, regrown with an eighth more when it
    // is too small.  nullptr when it cannot be had: see missing
    template <class T> T* get(u64 n) { keep.emplace_back(); return got<T>(keep.back(), keep.back().alloc(std::max<u64>(n, 1) * sizeof(T))); }
    template <class T> T* get(int id, u64 n) {
        if (!pool) pool = std::unique_lock<std::mutex>(g_cv_lock);
        DevBuf<>& b = g_cv[device * CV_N + id];
        const u64 need = std::max<u64>(n, 1) * sizeof(T);
        return got<T>(b, b.regrow(need, need / 8));
    }
    template <class T> T* got(const DevBuf<>& b, hipError_t e) { short_of |= e != hipSuccess; return e == hipSuccess ? b.as<T>() : nullptr; }
    // after a run of get: ECB_OK, or the refusal when one of them came back empty
    int missing() const { return short_of ? fail(nullptr, ECB_ERR_HIP, "%sout of device memory", prefix) : ECB_OK; }
    // n of the call's status words to the host, on its stream, and waited for; with a table, the error bits in word 0 refused
    int read_back(u64* host, const u64* words, u64 n) {
        CALLCHK(*this, hipMemcpyAsync(host, words, n * 8, hipMemcpyDeviceToHost, st));
        CALLCHK(*this, hipStreamSynchronize(st));
        return ECB_OK;
    }
    template <size_t N> int read_back(u64* host, const u64* words, u64 n, const ErrBit (&table)[N]) {
        const int r = read_back(host, words, n);
        return r != ECB_OK ? r : refuse_bits(nullptr, table, (u32)host[0]);
    }
    // the call's n status words -- the pool's, or with own = true a buffer of the call's --, zeroed, the first k of them all-ones: those are
    // lowest-offender words (NO_OFFENDER)
    int status_words(u64*& words, u64 n, u64 k, bool own = false) {
        words = own ? get<u64>(n) : get<u64>(CV_WORDS, n);
        if (const int r = missing()) return r;
        CALLCHK(*this, hipMemsetAsync(words, 0, n * 8, st));
        if (k) CALLCHK(*this, hipMemsetAsync(words, 0xFF, k * 8, st));
        return ECB_OK;
    }
};

// -- what the entry points below and the feature files (bus.inc, bus_correct.inc, strata.inc, umi.inc) share besides Call --
// every array in a fresh device buffer of max(bytes, 4) bytes (in list order), then the inputs copied in
struct StageIn { DevBuf<>* d; const void* src; u64 bytes; };          // (src null: an output, allocated only)
int stage_in(const Call& c, const std::vector<StageIn>& list) {
    for (const StageIn& a : list) CALLCHK(c, a.d->alloc(a.bytes, 4));
    for (const StageIn& a : list)
        if (a.src && a.bytes) CALLCHK(c, hipMemcpy(a.d->p, a.src, a.bytes, hipMemcpyHostToDevice));
    return ECB_OK;
}
// the results back: `bytes` of each (none when that is 0)
struct StageOut { void* dst; const DevBuf<>* d; u64 bytes; };
int stage_out(const Call& c, const std::vector<StageOut>& list) {
    for (const StageOut& a : list) if (a.bytes) CALLCHK(c, hipMemcpy(a.dst, a.d->p, a.bytes, hipMemcpyDeviceToHost));
    return ECB_OK;
}

// The lowest offender: every check that finds a breach does an atomicMin of (index << 8 | reason) on one status word, which only a
// refusal reads; the minimum does not depend on who arrives first.  NO_OFFENDER: nothing was found
constexpr u64 NO_OFFENDER = ~0ull;
__device__ __forceinline__ void offender(u64* err, u64 at, u32 reason) { atomicMin(reinterpret_cast<unsigned long long*>(err), (unsigned long long)(at << 8 | reason)); }
// the word read back: ECB_OK, or the refusal "<what> <index>: <reason>" (what: "bus: record")
int refuse_offender(u64 word, const char* what, const char* (*reason)(u32)) {
    if (word == NO_OFFENDER) return ECB_OK;
    return fail(nullptr, ECB_ERR_CONTRACT, "%s %llu: %s", what, (unsigned long long)(word >> 8), reason((u32)(word & 255u)));
}

// The tuple contract's step rule for the transforms of a tuple stream (strata.inc, umi.inc; the stream kernel checks tiles and sets error
// bits: k_stream.inc): 0, or why record `id` may not follow a record of `prev_id` -- the ids ascend in steps of 0 or 1, and a step lands
// on a record that passes the filter
enum : u32 { TUPLE_R_FALLS = 1, TUPLE_R_JUMPS, TUPLE_R_FILTERED };
const char* tuple_reason(u32 r) {
    switch (r) {
    case TUPLE_R_FALLS: return "read_id falls";
    case TUPLE_R_JUMPS: return "read_id steps by more than 1";
    case TUPLE_R_FILTERED: return "read_id steps on a record that does not pass the filter";
    default: return "unknown";
    }
}
__device__ __forceinline__ u32 tuple_step(u32 prev_id, u32 id, bool passes) {
    const u32 d = id - prev_id;
    if (d == 1u) return passes ? 0u : TUPLE_R_FILTERED;
    return d == 0u ? 0u : d < 0x80000000u ? TUPLE_R_JUMPS : TUPLE_R_FALLS;
}

// What has to outlive a sort is cut from ONE pool buffer, sized once from the input's bounds (thirty allocations of up to n words each per
// call cost more than the kernels: profiles/bus2ec_c4.txt).  A take beyond the room is refused, never handed out.
struct Arena {
    char* const p;
    const u64 cap;
    u64 used = 0;
    bool over = false;
    Arena(Call& c, int id, u64 cap_) : p(c.get<char>(id, cap_)), cap(cap_) {}
    static u64 pad(u64 n, u64 size) { return (std::max<u64>(n, 1) * size + 255ull) & ~255ull; }
    template <class T> T* take(u64 n) {
        const u64 b = pad(n, sizeof(T));
        if (!p || used + b > cap) { over = true; return nullptr; }
        T* q = reinterpret_cast<T*>(p + used);
        used += b;
        return q;
    }
    int missing(const Call& c) const { return over ? fail(nullptr, ECB_ERR_HIP, "%sthe scratch arena is too small (internal)", c.prefix) : c.missing(); }
};

// Caller memory that may not overlap.  Two byte ranges share a byte (an empty one shares none):
struct Span { const void* p; u64 bytes; };
bool spans_overlap(Span a, Span b) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
    return a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}
// ... and an entry point's arrays, the inputs first, the last n_out of them outputs: each output against every input, then against the
// outputs before it.  alias[k], where given: the input that output k may be exactly (the same first byte), -1: none
enum SpanClash { SPANS_APART, SPANS_OUT_IN, SPANS_OUT_OUT };
SpanClash span_clash(const std::vector<Span>& s, size_t n_out, const std::vector<int>& alias = {}) {
    const size_t n_in = s.size() - n_out;
    for (size_t o = n_in; o < s.size(); ++o)
        for (size_t j = 0; j < o; ++j) {
            if (o - n_in < alias.size() && alias[o - n_in] == (int)j && s[j].p == s[o].p) continue;
            if (spans_overlap(s[o], s[j])) return j < n_in ? SPANS_OUT_IN : SPANS_OUT_OUT;
        }
    return SPANS_APART;
}

const ErrBit CV_ERRS[] = {{~0u, ECB_ERR_CONTRACT, "malformed CSR: row pointers out of order, a locus beyond n_loci, or a mask that is zero or beyond n_haplotypes"}};
const ErrBit CVB_ERRS[] = {      // (CVB_ERR_ORDER is no refusal: the sort-everything path takes such a matrix)
    {CVB_ERR_PTR, ECB_ERR_CONTRACT, "malformed CSC: column pointers do not start at zero or go backwards"},
    {CVB_ERR_EC, ECB_ERR_CONTRACT, "malformed CSC: a row index beyond the number of ECs"},
};
// the general case: lists in any order, an EC more than once in a list -- every row index becomes a 64-bit key, all of them are sorted
// (rare, and as large as the matrix: in buffers of its own, not the pool's)
int hapcsc_to_csr_general(Call& c, u32 n_ecs, u32 n_loci, u32 n_haps, const void* d_cscptr, const void* d_cscidx, u64 total,
                          const std::vector<u64>& hs, void* d_indptr, void* d_indices, void* d_data, uint64_t* nnz_out) {
    hipStream_t st = c.st;
    u64 *d_hs = c.get<u64>(n_haps + 1), *keys = c.get<u64>(total), *keys2 = c.get<u64>(total);
    u32 *vals = c.get<u32>(total), *vals2 = c.get<u32>(total), *flag = c.get<u32>(total), *pos = c.get<u32>(total);
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemcpy(d_hs, hs.data(), (n_haps + 1) * 8, hipMemcpyHostToDevice));
    k_cv_back_expand<<<nblk(total, TPB), TPB, 0, st>>>((const int*)d_cscptr, (const int*)d_cscidx, total, n_loci, n_haps, d_hs, keys, vals);
    SortScratch ss{c.get<u32>(rs_words(total)), c.get<u32>(RS_AUX_WORDS), c.get<u64>(1)};
    u32* sums = c.get<u32>(scan_words(total) + 4);                  // (the scan's total behind its words)
    if (const int rc = c.missing()) return rc;
    u64* grand = reinterpret_cast<u64*>(sums + scan_words(total));
    SortBufs s{{keys, keys2}, {vals, vals2}};
    CALLCHK(c, radix_sort_pairs64(st, s, total, ss));
    k_run_heads<<<nblk(total, TPB), TPB, 0, st>>>(s.keys(), total, flag);
    u64 nnz = 0;
    CALLCHK(c, scan_launch(st, flag, total, pos, sums, grand));
    if (const int rc = c.read_back(&nnz, grand, 1)) return rc;
    k_cv_back_emit<<<nblk(total, TPB), TPB, 0, st>>>(s.keys(), s.vals(), flag, pos, total, n_loci, (int*)d_indices, (int*)d_data);
    k_cv_back_rowptr<<<nblk((u64)n_ecs + 1, TPB), TPB, 0, st>>>(s.keys(), pos, total, nnz, n_ecs, n_loci, (int*)d_indptr);
    CALLCHK(c, hipStreamSynchronize(st));
    *nnz_out = nnz;
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_release_scratch(int device) {
    if (device < 0 || device >= CV_MAX_DEV) return ECB_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, ECB_ERR_NO_DEVICE, "no such device");
    std::lock_guard<std::mutex> g(g_cv_lock);
    for (int i = 0; i < CV_N; ++i) g_cv[device * CV_N + i].reset();
    return ECB_OK;
}

namespace {
// both conversions CSR -> per-haplotype CSC: d_values / d_cscdata null = the incidence alone
int csr_to_hapcsc_any(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const void* d_indptr, const void* d_indices, const void* d_data,
                      const void* d_values, void* d_cscptr, void* d_cscidx, void* d_cscdata, bool payload, uint64_t* total) {
    if (!d_indptr || !total || !n_ecs || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if ((u64)n_haps * n_loci >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "haplotypes x loci does not fit 32 bits");
    Call c(device, ""); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    int nnz_i = 0;
    CALLCHK(c, hipMemcpy(&nnz_i, (const int*)d_indptr + n_ecs, 4, hipMemcpyDeviceToHost));
    if (nnz_i < 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSR: negative row pointer");
    const u64 nnz = (u64)nnz_i;
    if (nnz && (!d_indices || !d_data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");       // (a matrix without non-zeros has no arrays to point at)
    u64* words = c.get<u64>(CV_WORDS, 4);                          // [0] set bits, [1] the scan's total, [2] error bits
    if (const int rc = c.missing()) return rc;
    if (!d_cscidx || !d_cscptr || (payload && !d_cscdata)) {       // the first call: how many row indices there will be
        u64 tot = 0;
        CALLCHK(c, hipMemsetAsync(words, 0, 8, st));
        if (nnz) k_cv_bits<<<(unsigned)std::min<u64>(2048, nblk(nnz, TPB)), TPB, 0, st>>>((const int*)d_data, nnz, words);
        if (const int rc = c.read_back(&tot, words, 1)) return rc;
        if (tot >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
        *total = tot;
        return ECB_OK;
    }
    const u64 nc = (u64)n_haps * (n_loci + 1);
    if (!nnz) {
        CALLCHK(c, hipMemset(d_cscptr, 0, nc * 4));
        *total = 0;
        return ECB_OK;
    }
    const u32 nb = (u32)nblk(nnz, CVB);
    u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
    u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
    SortScratch ss{c.get<u32>(CV_HIST, rs_words(nnz)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 3};
    u32 *blk = c.get<u32>(CV_BLK, (u64)n_haps * nb), *scan = c.get<u32>(CV_SCAN, (u64)n_haps * nb);
    u32 *sums2 = c.get<u32>(CV_SUMS2, scan_words(std::max<u64>((u64)n_haps * nb, payload ? nnz + 1 : 0)) + 2);
    u32* headval = c.get<u32>(CV_HEAD, (u64)n_haps * n_loci);
    u32 *bits = nullptr, *bits_excl = nullptr, *base = nullptr;
    if (payload) { bits = c.get<u32>(CV_X0, nnz); bits_excl = c.get<u32>(CV_X1, nnz + 1); base = c.get<u32>(CV_X2, nnz); }
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemsetAsync(words, 0, 24, st));
    k_cv_keys<<<nblk(n_ecs, TPB), TPB, 0, st>>>((const int*)d_indptr, n_ecs, (const int*)d_indices, (const int*)d_data, nnz, n_loci, n_haps,
                                               k0, v0, reinterpret_cast<u32*>(words + 2));
    if (payload) {
        // the sort carries the non-zero's index in place of its mask; where each non-zero's values start: the scan of the popcounts
        k_iota<<<nblk(nnz, TPB), TPB, 0, st>>>(v0, nnz);
        k_cvv_bits<<<nblk(nnz, TPB), TPB, 0, st>>>((const int*)d_data, nnz, bits);
        CALLCHK(c, scan_launch(st, bits, nnz, bits_excl, sums2, nullptr, 1, bits_excl + nnz));
    }
    SortBufs s{{k0, k1}, {v0, v1}};
    // stable sort on the locus alone: ECs stay ascending within a column, as scipy's tocsc() leaves them
    CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_loci - 1) << 32));
    const u64* keys = s.keys(); const u32* masks = s.vals();
    if (payload) {
        u32* m2 = s.vals() == v0 ? v1 : v0;                         // (the sort's other value buffer is free now)
        k_cvv_gather<<<nblk(nnz, TPB), TPB, 0, st>>>(s.vals(), (const int*)d_data, bits_excl, nnz, m2, base);
        masks = m2;
    }
    k_cv_cnt<<<nb, TPB, 0, st>>>(masks, nnz, n_haps, nb, blk);
    CALLCHK(c, scan_launch(st, blk, (u64)n_haps * nb, scan, sums2, words + 1));
    u64 back[3] = {0, 0, 0};
    if (const int rc = c.read_back(back, words, 3)) return rc;
    if (const int rc = refuse_bits(nullptr, CV_ERRS, (u32)back[2])) return rc;
    if (back[1] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    *total = back[1];
    if (payload && back[1] && !d_values) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (payload)
        k_cv_emit<true><<<nb, TPB, 0, st>>>(keys, masks, nnz, n_haps, n_loci, nb, scan, (int*)d_cscidx, headval, base, (const double*)d_values,
                                            (double*)d_cscdata);
    else k_cv_emit<false><<<nb, TPB, 0, st>>>(keys, masks, nnz, n_haps, n_loci, nb, scan, (int*)d_cscidx, headval, nullptr, nullptr, nullptr);
    k_cv_ptr<<<nblk((u64)n_loci + 1, TPB), TPB, 0, st>>>(keys, nnz, n_loci, n_haps, nb, scan, words + 1, headval, (int*)d_cscptr);
    CALLCHK(c, hipStreamSynchronize(st));
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_csr_to_hapcsc_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const void* d_indptr,
                                        const void* d_indices, const void* d_data, void* d_cscptr, void* d_cscidx,
                                        uint64_t* total) {
    return csr_to_hapcsc_any(device, n_ecs, n_loci, n_haps, d_indptr, d_indices, d_data, nullptr, d_cscptr, d_cscidx, nullptr, false, total);
}

extern "C" int ecb_csr_to_hapcsc_values_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const void* d_indptr,
                                               const void* d_indices, const void* d_data, const void* d_values, void* d_cscptr,
                                               void* d_cscidx, void* d_cscdata, uint64_t* total) {
    return csr_to_hapcsc_any(device, n_ecs, n_loci, n_haps, d_indptr, d_indices, d_data, d_values, d_cscptr, d_cscidx, d_cscdata, true, total);
}

extern "C" int ecb_hapcsc_to_csr_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const void* d_cscptr,
                                        const void* d_cscidx, uint64_t total, void* d_indptr, void* d_indices, void* d_data,
                                        uint64_t* nnz_out) {
    if (!d_cscptr || !d_cscidx || !d_indptr || !d_indices || !d_data || !nnz_out || !n_ecs || !n_loci || !n_haps || n_haps > 31 || !total)
        return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (total >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 row indices");
    Call c(device, ""); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    // start of every haplotype's block = running sum of its last column pointer
    u64* words = c.get<u64>(CV_WORDS, 40);                          // [0] error bits  [1] the scan's total  [3] the sort's  [4 ..) last pointers, then block starts
    if (const int rc = c.missing()) return rc;
    int* d_last = reinterpret_cast<int*>(words + 4);
    std::vector<int> last(n_haps);
    k_cvb_last<<<1, 64, 0, st>>>((const int*)d_cscptr, n_loci, n_haps, d_last);
    CALLCHK(c, hipMemcpy(last.data(), d_last, n_haps * 4, hipMemcpyDeviceToHost));
    std::vector<u64> hs(n_haps + 1, 0);
    for (u32 h = 0; h < n_haps; ++h) {
        if (last[h] < 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSC: negative column pointer");
        hs[h + 1] = hs[h] + (u64)last[h];
    }
    if (hs[n_haps] != total) return fail(nullptr, ECB_ERR_ARG, "total does not match the column pointers");
    u64* d_hs = c.get<u64>(CV_X0, n_haps + 1);
    u32 *Ssum = c.get<u32>(CV_X1, (u64)n_loci + 1);
    u32 *colcnt = c.get<u32>(CV_HEAD, 5ull * n_loci + 8), *sums = c.get<u32>(CV_SUMS2, scan_words(n_loci) + 2);
    if (const int rc = c.missing()) return rc;
    u32 *colbase = colcnt + n_loci, *colcur = colbase + n_loci, *pieces = colcur + n_loci, *pbase = pieces + n_loci;
    u32* d_err = reinterpret_cast<u32*>(words);
    CALLCHK(c, hipMemcpyAsync(d_hs, hs.data(), (n_haps + 1) * 8, hipMemcpyHostToDevice, st));
    CALLCHK(c, hipMemsetAsync(words, 0, 24, st));
    CALLCHK(c, hipMemsetAsync(colcnt, 0, 3ull * n_loci * 4, st));
    k_cvu_colsum<<<nblk((u64)n_loci + 1, TPB), TPB, 0, st>>>((const int*)d_cscptr, n_loci, n_haps, Ssum, d_err);
    k_cvu_pieces<<<nblk(n_loci, TPB), TPB, 0, st>>>(Ssum, n_loci, pieces);
    CALLCHK(c, scan_launch(st, pieces, n_loci, pbase, sums, words + 2));
    u64 back[3] = {0, 0, 0};
    if (const int rc = c.read_back(back, words, 3, CVB_ERRS)) return rc;           // (CVB_ERR_PTR: nothing else has run)
    const u64 n_items = back[2];
    if (n_items == 0 || n_items >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "csc -> csr: pieces of work");
    u32 *item_col = c.get<u32>(CV_X2, n_items + 1), *bnd = c.get<u32>(CV_X3, (n_items + 1) * n_haps);
    if (const int rc = c.missing()) return rc;
    k_cvu_items<<<nblk(n_loci, TPB), TPB, 0, st>>>(pieces, pbase, n_loci, item_col);
    k_cvu_bounds<<<nblk(n_items * n_haps, TPB), TPB, 0, st>>>((const int*)d_cscptr, (const int*)d_cscidx, d_hs, pieces, pbase, item_col, (u32)n_items,
                                                             n_loci, n_haps, n_ecs, bnd);
    k_cvu_union<false><<<(unsigned)n_items, CVU_TPB, 0, st>>>((const int*)d_cscptr, (const int*)d_cscidx, d_hs, pieces, pbase, item_col, bnd, (u32)n_items,
                                                              n_loci, n_haps, n_ecs, colcnt, colbase, colcur, 0, nullptr, nullptr, d_err);
    CALLCHK(c, scan_launch(st, colcnt, n_loci, colbase, sums, words + 1));
    if (const int rc = c.read_back(back, words, 2, CVB_ERRS)) return rc;
    if ((u32)back[0] & CVB_ERR_ORDER)                              // a long column whose lists are not ascending: sort everything
        return hapcsc_to_csr_general(c, n_ecs, n_loci, n_haps, d_cscptr, d_cscidx, total, hs, d_indptr, d_indices, d_data, nnz_out);
    const u64 nnz = back[1];
    u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
    u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
    SortScratch ss{c.get<u32>(CV_HIST, rs_words(nnz)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 3};
    if (const int rc = c.missing()) return rc;
    k_cvu_union<true><<<(unsigned)n_items, CVU_TPB, 0, st>>>((const int*)d_cscptr, (const int*)d_cscidx, d_hs, pieces, pbase, item_col, bnd, (u32)n_items,
                                                             n_loci, n_haps, n_ecs, colcnt, colbase, colcur, nnz, k0, v0, d_err);
    SortBufs s{{k0, k1}, {v0, v1}};
    // stable, on the EC alone: what left column by column arrives row by row with its loci ascending
    CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_ecs - 1) << 32));
    k_split_out<<<nblk(nnz, TPB), TPB, 0, st>>>(s.keys(), s.vals(), nnz, (int*)d_indices, (int*)d_data);
    k_row_ptr<<<nblk((u64)n_ecs + 1, TPB), TPB, 0, st>>>(s.keys(), nnz, n_ecs, (int*)d_indptr);
    CALLCHK(c, hipStreamSynchronize(st));
    *nnz_out = nnz;
    return ECB_OK;
}

// ---- the same two conversions from and to HOST arrays: the library allocates, fills and frees its own device buffers, so a host
// that only converts files (alntools ec2emase / emase2ec, the .h5 writer of bam2emase: bin_utils.py:979-1028) needs no device
// allocator of its own -- and the Python drop-in no PyTorch on that path (stage_in / stage_out: next to Call).

extern "C" int ecb_csr_to_hapcsc(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const int32_t* indptr, const int32_t* indices,
                                 const int32_t* data, int32_t* csc_indptr, int32_t* csc_indices, uint64_t capacity, uint64_t* total) {
    if (!indptr || !total || !n_ecs || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    Call c(device, ""); if (c.rc) return c.rc;
    if (indptr[n_ecs] < 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSR: negative row pointer");
    const u64 nnz = (u64)indptr[n_ecs];
    if (nnz && (!indices || !data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (!csc_indices || !csc_indptr) {                 // the count alone: the set bits of the masks, on the host (one pass over nnz words)
        u64 tot = 0;
        for (u64 i = 0; i < nnz; ++i) tot += (u64)__builtin_popcount((unsigned)data[i]);
        if (tot >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
        *total = tot;
        return ECB_OK;
    }
    DevBuf<> ip, ix, da, cp, ci;
    const u64 nc = (u64)n_haps * (n_loci + 1);
    int rc = stage_in(c, {{&ip, indptr, ((u64)n_ecs + 1) * 4}, {&ix, indices, nnz * 4}, {&da, data, nnz * 4}, {&cp, nullptr, nc * 4},
                          {&ci, nullptr, capacity * 4}});
    // (the device entry point writes at most one row index per set bit: ask it for the count first when the caller's buffer might be short)
    uint64_t need = 0;
    if (rc == ECB_OK) rc = ecb_csr_to_hapcsc_device(device, n_ecs, n_loci, n_haps, ip.p, ix.p, da.p, nullptr, nullptr, &need);
    RCCHK(rc);
    *total = need;
    if (need > capacity) return fail(nullptr, ECB_ERR_ARG, "csc_indices holds %llu entries, the matrix has %llu set bits", (unsigned long long)capacity, (unsigned long long)need);
    RCCHK(ecb_csr_to_hapcsc_device(device, n_ecs, n_loci, n_haps, ip.p, ix.p, da.p, cp.p, ci.p, total));
    return stage_out(c, {{csc_indptr, &cp, nc * 4}, {csc_indices, &ci, *total * 4}});
}

extern "C" int ecb_csr_to_hapcsc_values(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const int32_t* indptr, const int32_t* indices,
                                        const int32_t* data, const double* values, int32_t* csc_indptr, int32_t* csc_indices, double* csc_data,
                                        uint64_t capacity, uint64_t* total) {
    if (!csc_indices || !csc_indptr || !csc_data)       // the count alone, as ecb_csr_to_hapcsc gives it
        return ecb_csr_to_hapcsc(device, n_ecs, n_loci, n_haps, indptr, indices, data, nullptr, nullptr, 0, total);
    if (!indptr || !total || !n_ecs || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    Call c(device, ""); if (c.rc) return c.rc;
    if (indptr[n_ecs] < 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSR: negative row pointer");
    const u64 nnz = (u64)indptr[n_ecs];
    if (nnz && (!indices || !data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    // the count first, on the host as ecb_csr_to_hapcsc takes it: nothing is allocated for a capacity the matrix does not need
    u64 need = 0;
    for (u64 i = 0; i < nnz; ++i) need += (u64)__builtin_popcount((unsigned)data[i]);
    if (need >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    *total = need;
    if (need > capacity) return fail(nullptr, ECB_ERR_ARG, "csc_indices holds %llu entries, the matrix has %llu set bits", (unsigned long long)capacity, (unsigned long long)need);
    if (need && !values) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    DevBuf<> ip, ix, da, va, cp, ci, cd;
    const u64 nc = (u64)n_haps * (n_loci + 1);
    RCCHK(stage_in(c, {{&ip, indptr, ((u64)n_ecs + 1) * 4}, {&ix, indices, nnz * 4}, {&da, data, nnz * 4}, {&va, values, need * 8}, {&cp, nullptr, nc * 4},
                       {&ci, nullptr, need * 4}, {&cd, nullptr, need * 8}}));
    RCCHK(ecb_csr_to_hapcsc_values_device(device, n_ecs, n_loci, n_haps, ip.p, ix.p, da.p, va.p, cp.p, ci.p, cd.p, total));
    return stage_out(c, {{csc_indptr, &cp, nc * 4}, {csc_indices, &ci, *total * 4}, {csc_data, &cd, *total * 8}});
}

extern "C" int ecb_hapcsc_to_csr(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, const int32_t* csc_indptr, const int32_t* csc_indices,
                                 uint64_t total, int32_t* indptr, int32_t* indices, int32_t* data, uint64_t* nnz) {
    if (!csc_indptr || !csc_indices || !indptr || !indices || !data || !nnz || !n_ecs || !n_loci || !n_haps || n_haps > 31 || !total)
        return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (total >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 row indices");
    Call c(device, ""); if (c.rc) return c.rc;
    DevBuf<> cp, ci, ip, ix, da;
    const u64 nc = (u64)n_haps * (n_loci + 1), rowb = ((u64)n_ecs + 1) * 4;
    int rc = stage_in(c, {{&cp, csc_indptr, nc * 4}, {&ci, csc_indices, total * 4}, {&ip, nullptr, rowb}, {&ix, nullptr, total * 4}, {&da, nullptr, total * 4}});
    if (rc == ECB_OK) rc = ecb_hapcsc_to_csr_device(device, n_ecs, n_loci, n_haps, cp.p, ci.p, total, ip.p, ix.p, da.p, nnz);
    RCCHK(rc);
    return stage_out(c, {{indptr, &ip, rowb}, {indices, &ix, *nnz * 4}, {data, &da, *nnz * 4}});
}

// ---- apply-genotypes: the haplotype bitmasks of a CSR A ANDed with a per-locus mask, what becomes zero dropped -----------------------------
// (AlignmentPropertyMatrix.apply_genotypes + ecsave2, AlignmentPropertyMatrix.py:483-505, Sparse3DMatrix.py:295-299: every non-zero of every
//  haplotype's matrix times gtmask[h, locus], zeros eliminated, rows kept.)  No loop over a row: three launches over the non-zeros -- a check
// that writes the keep flags, the one-pass scan of the flags, a scatter -- so rows of 1 and of 900 loci cost the same per non-zero.  The mask is
// a gather (T x 4 bytes: 320 KB at 80 k loci, L2-resident; it does not fit LDS).  Columns ascending within a row is checked without knowing
// the rows: a "descent" is a non-zero whose column is not above the one before it; the CSR is ascending exactly when every descent sits at
// the first non-zero of a row, i.e. when the descents the non-zeros count equal those the row pointers find at their rows' starts.
namespace {
constexpr int GM_ITEMS = 4;                            // non-zeros per thread (16-byte loads)
constexpr u32 GM_SHARDS = 256, GM_SHARD_WORDS = 16;    // descent balance: 256 counters, one 128-byte line each
enum : u32 { GM_ERR_PTR = 1u, GM_ERR_LOCUS = 2u, GM_ERR_BITS = 4u, GM_ERR_MASK = 8u, GM_SAW_ZERO = 16u };      // (GM_SAW_ZERO is no error: GM_ERRS does not list it)
// words: [0] error bits, [3] kept non-zeros (the scan's total), then from word 16 the shards: shard s at word 16 + 16 s holds, summed over
// the workgroups b with b % 256 == s, (descents among the non-zeros) - (descents at a row's first non-zero), mod 2^64.  The balance of the
// whole CSR is 0 exactly when it is ascending.  (One counter for the whole grid took every wave's add: 1.3 ms at 13 M non-zeros.)
// thread t: row pointer t (t <= E), mask word t (t < T), non-zeros [4t, 4t + 4) (< nnz)
// COUNT: the same check for count-alignments, which has no mask: keep[i] = the set bits of non-zero i, and GM_SAW_ZERO when one holds none
template <bool COUNT>
__global__ __launch_bounds__(TPB) void k_gm_check(const int* indptr, u32 n_ecs, const int* indices, const int* data, u64 nnz, const u32* mask,
                                                  u32 n_loci, u32 n_haps, u32* keep, u64* words) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    u32 err = 0, desc = 0, desc_row = 0;
    if (t <= n_ecs) {
        const long long a = indptr[t];
        if (a < 0 || (u64)a > nnz || (t == 0 && a != 0) || (t == n_ecs && (u64)a != nnz)) err |= GM_ERR_PTR;
        else if (t < n_ecs) {
            const long long b = indptr[t + 1];
            if (b < a || (u64)b > nnz) err |= GM_ERR_PTR;
            else if (b > a && a > 0 && (u32)indices[a] <= (u32)indices[a - 1]) desc_row = 1;
        }
    }
    if (!COUNT && t < n_loci && (mask[t] >> n_haps) != 0u) err |= GM_ERR_MASK;
    const u64 i0 = t * GM_ITEMS;
    if (i0 < nnz) {
        u32 c[GM_ITEMS], d[GM_ITEMS], k[GM_ITEMS];
        const bool whole = i0 + GM_ITEMS <= nnz;
        if (whole && ((reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(data) | reinterpret_cast<uintptr_t>(keep)) & 15u) == 0u) {
            const uint4 q = reinterpret_cast<const uint4*>(indices + i0)[0], r = reinterpret_cast<const uint4*>(data + i0)[0];
            c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w; d[0] = r.x; d[1] = r.y; d[2] = r.z; d[3] = r.w;
        } else {
#pragma unroll
            for (int j = 0; j < GM_ITEMS; ++j) { c[j] = i0 + j < nnz ? (u32)indices[i0 + j] : 0u; d[j] = i0 + j < nnz ? (u32)data[i0 + j] : 0u; }
        }
        u32 prev = i0 ? (u32)indices[i0 - 1] : 0u;
#pragma unroll
        for (int j = 0; j < GM_ITEMS; ++j) {
            k[j] = 0u;
            if (i0 + j >= nnz) continue;
            if (i0 + j > 0 && c[j] <= prev) ++desc;
            prev = c[j];
            if ((d[j] >> n_haps) != 0u) err |= GM_ERR_BITS;
            if (c[j] >= n_loci) err |= GM_ERR_LOCUS;
            else if (COUNT) { k[j] = (u32)__popc(d[j]); if (!d[j]) err |= GM_SAW_ZERO; }
            else k[j] = (d[j] & mask[c[j]]) != 0u;
        }
        if (whole && (reinterpret_cast<uintptr_t>(keep) & 15u) == 0u) reinterpret_cast<uint4*>(keep + i0)[0] = make_uint4(k[0], k[1], k[2], k[3]);
        else {
#pragma unroll
            for (int j = 0; j < GM_ITEMS; ++j) if (i0 + j < nnz) keep[i0 + j] = k[j];
        }
    }
    // (every lane of the workgroup gets here: the wave sums and the barrier need them all)
    if (err) atomicOr(reinterpret_cast<u32*>(words), err);
    __shared__ long long s_bal[TPB / 64];
    const long long bal = (long long)wave_sum(desc) - (long long)wave_sum(desc_row);
    if ((threadIdx.x & 63u) == 0u) s_bal[threadIdx.x >> 6] = bal;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long b = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) b += s_bal[w];
        if (b) atomicAdd(reinterpret_cast<unsigned long long*>(words + GM_SHARD_WORDS * (1 + blockIdx.x % GM_SHARDS)), (unsigned long long)b);
    }
}
// excl = exclusive scan of keep, nnz + 1 values (excl[nnz] = kept): non-zero i is kept when excl[i + 1] != excl[i] and goes to excl[i];
// row e starts at excl[indptr[e]].  Every write stays inside its array whatever the input held (and a malformed CSR never gets here: the
// call reads the check's verdict first, so that a refused call leaves the caller's outputs as they were).
__global__ __launch_bounds__(TPB) void k_gm_scatter(const int* indptr, u32 n_ecs, const int* indices, const int* data, u64 nnz, const u32* mask,
                                                    u32 n_loci, const u32* excl, int* out_indptr, int* out_indices, int* out_data) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t <= n_ecs) {
        const long long a = indptr[t];
        out_indptr[t] = a >= 0 && (u64)a <= nnz ? (int)excl[a] : 0;
    }
    const u64 i0 = t * GM_ITEMS;
    if (i0 >= nnz) return;
    u32 c[GM_ITEMS], d[GM_ITEMS], x[GM_ITEMS + 1];
    if (i0 + GM_ITEMS <= nnz && ((reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(data) | reinterpret_cast<uintptr_t>(excl)) & 15u) == 0u) {
        const uint4 q = reinterpret_cast<const uint4*>(indices + i0)[0], r = reinterpret_cast<const uint4*>(data + i0)[0];
        const uint4 s = reinterpret_cast<const uint4*>(excl + i0)[0];
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w; d[0] = r.x; d[1] = r.y; d[2] = r.z; d[3] = r.w;
        x[0] = s.x; x[1] = s.y; x[2] = s.z; x[3] = s.w; x[4] = excl[i0 + GM_ITEMS];
    } else {
#pragma unroll
        for (int j = 0; j < GM_ITEMS; ++j) {
            c[j] = i0 + j < nnz ? (u32)indices[i0 + j] : 0u; d[j] = i0 + j < nnz ? (u32)data[i0 + j] : 0u;
            x[j] = i0 + j <= nnz ? excl[i0 + j] : 0u;
        }
        x[GM_ITEMS] = i0 + GM_ITEMS <= nnz ? excl[i0 + GM_ITEMS] : 0u;
    }
#pragma unroll
    for (int j = 0; j < GM_ITEMS; ++j) {
        if (i0 + j >= nnz || x[j + 1] == x[j] || c[j] >= n_loci) continue;
        out_indices[x[j]] = (int)c[j];
        out_data[x[j]] = (int)(d[j] & mask[c[j]]);
    }
}
const ErrBit GM_ERRS[] = {
    {GM_ERR_PTR, ECB_ERR_CONTRACT, "malformed CSR: row pointers do not start at 0, go backwards or do not end at nnz"},
    {GM_ERR_LOCUS, ECB_ERR_CONTRACT, "malformed CSR: a locus at or beyond n_loci"},
    {GM_ERR_BITS, ECB_ERR_CONTRACT, "malformed CSR: a haplotype bit at or beyond n_haplotypes"},
    {GM_ERR_MASK, ECB_ERR_CONTRACT, "a locus mask has a bit at or beyond n_haplotypes"},
};
}  // namespace

extern "C" int ecb_apply_mask_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr,
                                     const void* d_indices, const void* d_data, const void* d_mask, void* d_out_indptr, void* d_out_indices,
                                     void* d_out_data, uint64_t* kept) {
    if (!d_indptr || !d_mask || !d_out_indptr || !kept || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (nnz && (!d_indices || !d_data || !d_out_indices || !d_out_data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (nnz >= (1ull << 31) || n_ecs >= (1u << 31) - 1u) return fail(nullptr, ECB_ERR_LIMIT, "the CSR exceeds the .bin format's int32 limits");
    const u64 rowb = ((u64)n_ecs + 1) * 4, nzb = nnz * 4;
    if (const SpanClash clash = span_clash({{d_indptr, rowb}, {d_indices, nzb}, {d_data, nzb}, {d_mask, (u64)n_loci * 4}, {d_out_indptr, rowb},
                                            {d_out_indices, nzb}, {d_out_data, nzb}}, 3))
        return fail(nullptr, ECB_ERR_ARG, "%s", clash == SPANS_OUT_IN ? "an output overlaps an input" : "the outputs overlap");
    Call c(device, "apply-mask: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *keep = c.get<u32>(CV_X0, nnz), *excl = c.get<u32>(CV_X1, nnz + 1), *sums = c.get<u32>(CV_SUMS2, scan_words(nnz));
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemsetAsync(words, 0, n_words * 8, st));
    const u64 threads = std::max<u64>(std::max<u64>((u64)n_ecs + 1, n_loci), (nnz + GM_ITEMS - 1) / GM_ITEMS);
    const int* ip = (const int*)d_indptr; const int* ix = (const int*)d_indices; const int* da = (const int*)d_data; const u32* mk = (const u32*)d_mask;
    k_gm_check<false><<<nblk(threads, TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, mk, n_loci, n_haps, keep, words);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, keep, nnz, excl, sums, words + 3, 1, excl + nnz));
    // the verdict first: a refused call writes nothing into the caller's outputs (one more wait; the scatter is then a launch of its own)
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    u64 balance = 0;
    for (u32 k = 1; k <= GM_SHARDS; ++k) balance += back[GM_SHARD_WORDS * k];
    if (balance != 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSR: columns not strictly ascending within a row (unsorted or duplicate)");
    k_gm_scatter<<<nblk(threads, TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, mk, n_loci, excl, (int*)d_out_indptr, (int*)d_out_indices, (int*)d_out_data);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, hipStreamSynchronize(st));
    *kept = back[3];
    return ECB_OK;
}

extern "C" int ecb_apply_mask(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr, const int32_t* indices,
                              const int32_t* data, const uint32_t* mask, int32_t* out_indptr, int32_t* out_indices, int32_t* out_data, uint64_t* kept) {
    if (!indptr || !mask || !out_indptr || !kept || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (nnz && (!indices || !data || !out_indices || !out_data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (nnz >= (1ull << 31) || n_ecs >= (1u << 31) - 1u) return fail(nullptr, ECB_ERR_LIMIT, "the CSR exceeds the .bin format's int32 limits");
    Call c(device, "apply-mask: "); if (c.rc) return c.rc;
    const u64 rowb = ((u64)n_ecs + 1) * 4, nzb = nnz * 4;
    DevBuf<> ip, ix, da, mk, oip, oix, oda;
    int rc = stage_in(c, {{&ip, indptr, rowb}, {&ix, indices, nzb}, {&da, data, nzb}, {&mk, mask, (u64)n_loci * 4}, {&oip, nullptr, rowb},
                          {&oix, nullptr, nzb}, {&oda, nullptr, nzb}});
    if (rc == ECB_OK) rc = ecb_apply_mask_device(device, n_ecs, n_loci, n_haps, nnz, ip.p, ix.p, da.p, mk.p, oip.p, oix.p, oda.p, kept);
    RCCHK(rc);
    return stage_out(c, {{out_indptr, &oip, rowb}, {out_indices, &oix, *kept * 4}, {out_data, &oda, *kept * 4}});
}

// ---- count-alignments: per-target read counts of a CSR A weighted by N (ecb_count_alignments / ecb_count_alignments_device) --------------
// (AlignmentPropertyMatrix.count_alignments / count_unique_reads, AlignmentPropertyMatrix.py:429-448.)  A weighted scatter-add of every set
// bit onto 2 H T + T int64 counters.  Global atomics run at the memory side, one 64-byte request per scattered lane (MI355X: a set bit each
// would be ~30 M requests at config 3), so the non-zeros are first put in the order of their locus WINDOW -- CA window loci whose
// (2 H + 1) x 8-byte counters fit LDS -- by ONE pass of the library's radix sort (the window number is a digit of its own in the key),
// and a workgroup then adds a stretch of that order into LDS and sends each counter it touched to memory once, as consecutive 8-byte adds.
// No loop over a row: the weight and the two row flags travel as one word per EC (ww), the flags from prefix sums over the non-zeros, and
// the key pass finds a non-zero's row by bisecting the row pointers between its workgroup's first and last row.
// Steps: k_ca_weights (N -> ww, N checked) | k_gm_check<true> (apply-mask's CSR check; set bits per non-zero) | k_scan_lb | [zero masks
// present: k_ca_nonzero, k_scan_lb] | k_ca_rows | k_ca_keys | k_rs_* (one pass per 8 bits of window number) | k_ca_accum.
namespace {
constexpr u32 CA_LDS_BYTES = 80u << 10;              // of the window's counters: two workgroups per CU
constexpr u32 CA_TPB = 512, CA_CHUNK = 32768;        // k_ca_accum: threads, and sorted non-zeros per workgroup
constexpr u32 CA_KEY_ITEMS = 4;                      // k_ca_keys: non-zeros per thread
constexpr u32 CA_WIN_SHIFT = 40;                     // key = window << 40 | locus within the window << H | mask   (H + log2 window <= 38)
constexpr u64 CA_LEN1 = 1ull << 63, CA_POP1 = 1ull << 62, CA_WEIGHT = CA_POP1 - 1ull;      // ww[e]: row flags over the weight (< 2^62)
enum : u32 { CA_ERR_NPTR = 1u, CA_ERR_EC = 2u, CA_ERR_NEG = 4u };
// log2 of the loci per window: the largest power of two whose 2 H + 1 counters per locus fit CA_LDS_BYTES (H = 31: 128 loci, H = 1: 2048)
inline u32 ca_window_bits(u32 n_haps) {
    const u32 fit = CA_LDS_BYTES / 8u / (2u * n_haps + 1u);
    return 31u - (u32)__builtin_clz(fit);
}
// what is wrong with column pointer j of N (j <= S) and with its entry j (j < nnz_n): CA_ERR_* bits (count-alignments and ecselect)
__device__ __forceinline__ u32 ca_n_errors(u64 j, const int* indptr_n, u32 n_samples, const int* indices_n, const int* data_n, u64 nnz_n, u32 n_ecs) {
    u32 err = 0;
    if (j <= n_samples) {
        const long long a = indptr_n[j];
        if (a < 0 || (u64)a > nnz_n || (j == 0 && a != 0) || (j == n_samples && (u64)a != nnz_n)) err |= CA_ERR_NPTR;
        else if (j < n_samples && indptr_n[j + 1] < a) err |= CA_ERR_NPTR;
    }
    if (j < nnz_n) {
        const int e = indices_n[j];
        if (e < 0 || (u32)e >= n_ecs) err |= CA_ERR_EC;
        else if (data_n[j] < 0) err |= CA_ERR_NEG;
    }
    return err;
}
// thread j: column pointer j of N (j <= S) and entry j (j < nnz_n): everything checked, the entries of the sample(s) asked for added to ww
__global__ __launch_bounds__(TPB) void k_ca_weights(const int* indptr_n, u32 n_samples, const int* indices_n, const int* data_n, u64 nnz_n,
                                                    u32 n_ecs, long long sample, u64* ww, u64* words) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    const u32 err = ca_n_errors(j, indptr_n, n_samples, indices_n, data_n, nnz_n, n_ecs);
    if (j < nnz_n && !(err & (CA_ERR_EC | CA_ERR_NEG))) {
        const int e = indices_n[j], c = data_n[j];
        if (c > 0 && (sample < 0 || ((long long)j >= indptr_n[sample] && (long long)j < indptr_n[sample + 1])))
            atomicAdd(reinterpret_cast<unsigned long long*>(ww + e), (unsigned long long)c);
    }
    if (err) atomicOr(reinterpret_cast<u32*>(words + 1), err);
}
// bits[i] = set bits of non-zero i  ->  1 where it has any (in place: the second prefix sum, taken only when a mask of 0 was seen)
__global__ __launch_bounds__(TPB) void k_ca_nonzero(u32* bits, u64 nnz) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < nnz) bits[i] = bits[i] != 0u;
}
// row e: CA_POP1 when its masks hold one set bit in all, CA_LEN1 when one of its non-zeros has a mask other than 0 (nz_excl null: no mask
// is 0, and that is the row's length); excl arrays are exclusive prefix sums with nnz + 1 values
// (the classifier itself, shared with ecselect: pop = the set bits of row e's masks, nzc = its non-zeros whose mask is not 0; both 0 for an
//  empty row)
__device__ __forceinline__ void ca_row_counts(const int* indptr, u64 e, u64 nnz, const u32* bits_excl, const u32* nz_excl, u32& pop, u32& nzc) {
    pop = nzc = 0;
    const long long a = indptr[e], b = indptr[e + 1];
    if (a < 0 || b <= a || (u64)b > nnz) return;
    pop = bits_excl[b] - bits_excl[a];
    nzc = nz_excl ? nz_excl[b] - nz_excl[a] : (u32)(b - a);
}
__global__ __launch_bounds__(TPB) void k_ca_rows(const int* indptr, u32 n_ecs, u64 nnz, const u32* bits_excl, const u32* nz_excl, u64* ww) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e >= n_ecs) return;
    u32 pop, nzc;
    ca_row_counts(indptr, e, nnz, bits_excl, nz_excl, pop, nzc);
    u64 f = 0;
    if (pop == 1u) f |= CA_POP1;
    if (nzc == 1u) f |= CA_LEN1;
    if (f) ww[e] |= f;
}
// the last row of [lo, hi] whose pointer is at or below i (row pointers never fall: checked before this runs)
__device__ __forceinline__ u32 ca_row_of(const int* indptr, u32 lo, u32 hi, u64 i) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if ((u64)(u32)indptr[mid] <= i) lo = mid; else hi = mid - 1u;
    }
    return lo;
}
// the rows that hold a workgroup's first and last entry (b0, b1), found once per workgroup: every thread of it calls this
__device__ __forceinline__ void ca_block_rows(const int* indptr, u32 n_rows, u64 b0, u64 b1, u32* s_row) {
    if (threadIdx.x == 0) s_row[0] = ca_row_of(indptr, 0, n_rows - 1, b0);
    if (threadIdx.x == 64) s_row[1] = ca_row_of(indptr, 0, n_rows - 1, b1);
    __syncthreads();
}
// thread t: non-zeros [4t, 4t + 4) -> key (window, locus within it, mask) and value (row)
__global__ __launch_bounds__(TPB) void k_ca_keys(const int* indptr, u32 n_ecs, const int* indices, const int* data, u64 nnz, u32 lgw, u32 n_haps,
                                                 u64* keys, u32* rows) {
    __shared__ u32 s_row[2];
    const u64 b0 = blockIdx.x * (u64)(TPB * CA_KEY_ITEMS), b1 = std::min<u64>(nnz, b0 + TPB * CA_KEY_ITEMS) - 1;
    ca_block_rows(indptr, n_ecs, b0, b1, s_row);
    const u64 i0 = b0 + (u64)threadIdx.x * CA_KEY_ITEMS;
    if (i0 >= nnz) return;
    const u32 hi = s_row[1];
    u32 r = ca_row_of(indptr, s_row[0], hi, i0);
#pragma unroll
    for (u32 j = 0; j < CA_KEY_ITEMS; ++j) {
        const u64 i = i0 + j;
        if (i >= nnz) break;
        if (r < hi && (u64)(u32)indptr[r + 1] <= i) r = ca_row_of(indptr, r + 1, hi, i);
        const u32 t = (u32)indices[i];
        keys[i] = (u64)(t >> lgw) << CA_WIN_SHIFT | (u64)(t & ((1u << lgw) - 1u)) << n_haps | (u32)data[i];
        rows[i] = r;
    }
}
// workgroup b: sorted non-zeros [b CA_CHUNK, (b + 1) CA_CHUNK), one window's stretch at a time: its counters zeroed in LDS (planes aln[H],
// uniq[H], locus_uniq, each a window wide), every set bit added there, then every counter that is not 0 added to memory.  A counter is thus
// sent once per (workgroup, window): at most nnz / CA_CHUNK + windows times the table, in runs of consecutive addresses.
__global__ __launch_bounds__(CA_TPB) void k_ca_accum(const u64* keys, const u32* rows, u64 nnz, const u64* ww, u32 n_loci, u32 n_haps, u32 lgw,
                                                     long long* aln, long long* uniq, long long* locus_uniq) {
    extern __shared__ u64 s_tab[];
    const u32 W = 1u << lgw, n_tab = W * (2u * n_haps + 1u), tid = threadIdx.x;
    const u64 hmask = (1ull << n_haps) - 1ull;
    const u64 c0 = blockIdx.x * (u64)CA_CHUNK, c1 = std::min<u64>(nnz, c0 + CA_CHUNK);
    for (u64 pos = c0; pos < c1;) {
        const u64 win = keys[pos] >> CA_WIN_SHIFT;
        u64 lo = pos, end = c1;                      // keys[lo] is of this window; keys[end] is not, or end = c1
        while (lo + 1 < end) {
            const u64 mid = (lo + end) / 2;
            if ((keys[mid] >> CA_WIN_SHIFT) == win) lo = mid; else end = mid;
        }
        for (u32 k = tid; k < n_tab; k += CA_TPB) s_tab[k] = 0;
        __syncthreads();
        for (u64 i = pos + tid; i < end; i += CA_TPB) {
            const u64 key = keys[i], g = ww[rows[i]], w = g & CA_WEIGHT;
            u32 m = (u32)(key & hmask);
            if (!w || !m) continue;
            const u32 lw = (u32)(key >> n_haps) & (W - 1u);
            if (g & CA_LEN1) atomicAdd(reinterpret_cast<unsigned long long*>(&s_tab[2u * n_haps * W + lw]), (unsigned long long)w);
            for (; m; m &= m - 1u) {
                const u32 h = (u32)__ffs((int)m) - 1u;
                atomicAdd(reinterpret_cast<unsigned long long*>(&s_tab[h * W + lw]), (unsigned long long)w);
                if (g & CA_POP1) atomicAdd(reinterpret_cast<unsigned long long*>(&s_tab[(n_haps + h) * W + lw]), (unsigned long long)w);
            }
        }
        __syncthreads();
        for (u32 k = tid; k < n_tab; k += CA_TPB) {
            const u64 v = s_tab[k];
            const u64 t = (win << lgw) + (k & (W - 1u));
            if (!v || t >= n_loci) continue;
            const u32 plane = k >> lgw;
            long long* dst = plane < n_haps ? aln : plane < 2u * n_haps ? uniq : locus_uniq;
            const u32 h = plane < n_haps ? plane : plane < 2u * n_haps ? plane - n_haps : 0u;
            if (dst) atomicAdd(reinterpret_cast<unsigned long long*>(dst + (u64)h * n_loci + t), (unsigned long long)v);
        }
        __syncthreads();
        pos = end;
    }
}
const ErrBit CA_ERRS[] = {
    {CA_ERR_NPTR, ECB_ERR_CONTRACT, "malformed N: column pointers do not start at 0, go backwards or do not end at nnz_n"},
    {CA_ERR_EC, ECB_ERR_CONTRACT, "malformed N: an EC index at or beyond n_ecs"},
    {CA_ERR_NEG, ECB_ERR_CONTRACT, "malformed N: a negative count"},
};
// the pointers and sizes of A and N that count-alignments and ecselect refuse before anything is allocated
int ca_check_matrices(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* indptr_a, const void* indices_a, const void* data_a,
                      uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n) {
    if (!indptr_a || !indptr_n || !n_loci || !n_haps || n_haps > 31 || !n_samples) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if ((nnz_a && (!indices_a || !data_a)) || (nnz_n && (!indices_n || !data_n))) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (n_ecs >= (1u << 31) - 1u || nnz_n >= (1ull << 31) || n_samples >= (1u << 31) - 1u)
        return fail(nullptr, ECB_ERR_LIMIT, "the matrices exceed the .bin format's int32 limits");
    return ECB_OK;
}
// the status words of k_gm_check<true> and of the check of N, read back: the refusal of a malformed A or N (the error bits of A in word 0
// have been refused by read_back), or ECB_OK
int ca_refuse_input(const std::vector<u64>& back) {
    u64 balance = 0;
    for (u32 k = 1; k <= GM_SHARDS; ++k) balance += back[GM_SHARD_WORDS * k];
    if (balance != 0) return fail(nullptr, ECB_ERR_CONTRACT, "malformed CSR: columns not strictly ascending within a row (unsorted or duplicate)");
    return refuse_bits(nullptr, CA_ERRS, (u32)back[1]);
}
// what both entry points refuse before anything is allocated
int ca_check_args(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* indptr_a, const void* indices_a, const void* data_a,
                  uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int64_t sample) {
    RCCHK(ca_check_matrices(n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n));
    if (nnz_a >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "count-alignments: 2^30 non-zeros or more");       // (radix_sort_pairs64)
    if (sample < -1 || sample >= (int64_t)n_samples) return fail(nullptr, ECB_ERR_CONTRACT, "count-alignments: no such sample (%lld of %u)", (long long)sample, n_samples);
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_count_alignments_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                           const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                           const void* d_indices_n, const void* d_data_n, int64_t sample, void* d_aln, void* d_uniq,
                                           void* d_locus_uniq) {
    RCCHK(ca_check_args(n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, sample));
    Call c(device, "count-alignments: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);          // apply-mask's words; [1] the error bits of N, [2] the second scan's total
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *bits = c.get<u32>(CV_X0, nnz), *bits_excl = c.get<u32>(CV_X1, nnz + 1), *sums = c.get<u32>(CV_SUMS2, scan_words(nnz));
    u64* ww = c.get<u64>(CV_X2, n_ecs);
    if (const int rc = c.missing()) return rc;
    const int* ip = (const int*)d_indptr_a; const int* ix = (const int*)d_indices_a; const int* da = (const int*)d_data_a;
    CALLCHK(c, hipMemsetAsync(words, 0, n_words * 8, st));
    CALLCHK(c, hipMemsetAsync(ww, 0, std::max<u64>(n_ecs, 1) * 8, st));
    k_ca_weights<<<nblk(std::max<u64>(nnz_n, (u64)n_samples + 1), TPB), TPB, 0, st>>>((const int*)d_indptr_n, n_samples, (const int*)d_indices_n,
                                                                                     (const int*)d_data_n, nnz_n, n_ecs, sample, ww, words);
    k_gm_check<true><<<nblk(std::max<u64>((u64)n_ecs + 1, (nnz + GM_ITEMS - 1) / GM_ITEMS), TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, nullptr, n_loci,
                                                                                                             n_haps, bits, words);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, bits, nnz, bits_excl, sums, words + 3, 1, bits_excl + nnz));
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    if (back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    // the input is well formed: from here on the outputs are written
    u32* nz_excl = nullptr;
    if ((u32)back[0] & GM_SAW_ZERO) {
        nz_excl = c.get<u32>(CV_X3, nnz + 1);
        if (const int rc = c.missing()) return rc;
        k_ca_nonzero<<<nblk(nnz, TPB), TPB, 0, st>>>(bits, nnz);
        CALLCHK(c, scan_launch(st, bits, nnz, nz_excl, sums, words + 2, 1, nz_excl + nnz));
    }
    if (n_ecs) k_ca_rows<<<nblk(n_ecs, TPB), TPB, 0, st>>>(ip, n_ecs, nnz, bits_excl, nz_excl, ww);
    const u64 plane = (u64)n_haps * n_loci * 8;
    if (d_aln) CALLCHK(c, hipMemsetAsync(d_aln, 0, plane, st));
    if (d_uniq) CALLCHK(c, hipMemsetAsync(d_uniq, 0, plane, st));
    if (d_locus_uniq) CALLCHK(c, hipMemsetAsync(d_locus_uniq, 0, (u64)n_loci * 8, st));
    if (nnz) {
        const u32 lgw = ca_window_bits(n_haps);
        u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
        u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
        SortScratch ss{c.get<u32>(CV_HIST, rs_words(nnz)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 4};
        if (const int rc = c.missing()) return rc;
        k_ca_keys<<<nblk(nnz, TPB * CA_KEY_ITEMS), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, lgw, n_haps, k0, v0);
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask((u64)(n_loci - 1) >> lgw) << CA_WIN_SHIFT));
        const u32 lds = ((2u * n_haps + 1u) << lgw) * 8u;
        // (more than the 64 KB a kernel may take unasked; per device, so asked for on every call)
        CALLCHK(c, hipFuncSetAttribute((const void*)k_ca_accum, hipFuncAttributeMaxDynamicSharedMemorySize, CA_LDS_BYTES));
        k_ca_accum<<<nblk(nnz, CA_CHUNK), CA_TPB, lds, st>>>(s.keys(), s.vals(), nnz, ww, n_loci, n_haps, lgw, (long long*)d_aln, (long long*)d_uniq,
                                                             (long long*)d_locus_uniq);
        CALLCHK(c, hipGetLastError());
    }
    CALLCHK(c, hipStreamSynchronize(st));
    return ECB_OK;
}

extern "C" int ecb_count_alignments(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                                    const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                    const int32_t* indices_n, const int32_t* data_n, int64_t sample, int64_t* aln, int64_t* uniq, int64_t* locus_uniq) {
    RCCHK(ca_check_args(n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n, sample));
    Call c(device, "count-alignments: "); if (c.rc) return c.rc;
    const u64 plane = (u64)n_haps * n_loci * 8;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, oa, ou, ol;
    std::vector<StageIn> in = {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz * 4}, {&daa, data_a, nnz * 4},
                               {&ipn, indptr_n, ((u64)n_samples + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4}};
    if (aln) in.push_back({&oa, nullptr, plane});
    if (uniq) in.push_back({&ou, nullptr, plane});
    if (locus_uniq) in.push_back({&ol, nullptr, (u64)n_loci * 8});
    int rc = stage_in(c, in);
    if (rc == ECB_OK) rc = ecb_count_alignments_device(device, n_ecs, n_loci, n_haps, nnz, ipa.p, ixa.p, daa.p, n_samples, nnz_n, ipn.p, ixn.p, dan.p,
                                                       sample, oa.p, ou.p, ol.p);
    RCCHK(rc);
    return stage_out(c, {{aln, &oa, aln ? plane : 0}, {uniq, &ou, uniq ? plane : 0}, {locus_uniq, &ol, locus_uniq ? (u64)n_loci * 8 : 0}});
}

// ecquant (ecb_quantify / ecb_quantify_device): the EM on count-alignments' checks and weights and the conversion's column order
#include "quant.inc"
// ... and its hierarchical models over a gene grouping (ecb_quantify_model / ecb_quantify_model_device)
#include "quant_model.inc"
// ... and one EM per cell of a multisample N, batched (ecb_cell_support* / ecb_quantify_cells*)
#include "quant_cells.inc"
// ... and the hierarchical models per cell (ecb_quantify_cells_model*)
#include "quant_cells_model.inc"
// ... and the posterior of every alignment at a given theta (ecb_posterior*)
#include "quant_post.inc"
// ... and bootstrap replicates of N and the moments of their estimates (ecb_resample* / ecb_quantify_bootstrap*)
#include "boot_draw.h"
#include "boot.inc"
// the connected components of the target-EC incidence, on count-alignments' checks and weights (ecb_components / ecb_components_device)
#include "components.inc"

// ---- ecselect: the reads of one class and the samples that still count enough of them, pulled out of a .bin (ecb_select / ecb_select_device)
// (AlignmentPropertyMatrix.get_unique_reads / pull_alignments_from, AlignmentPropertyMatrix.py:386-427, and the cell threshold of
//  bam2ec --multisample, bam_utils_multisample.py:596-636.)  Linear passes only, no loop over a row or a column: the row flags come from
// count-alignments' classifier (prefix sums of popcounts over the non-zeros), a pass over N adds up the per-sample totals (a wave whose
// entries all lie in one column sends one int64 add), a second pass over N marks the entries that stay and, with plain stores, the rows they
// keep alive; four scans give the new row numbers, the new row pointers of A, the new places of N's entries and the new sample numbers;
// two gathers copy.  Nothing is written to the caller's arrays before the input has been found well formed.
// Steps: k_sel_ncheck | k_gm_check<true> | [a class: k_scan_lb] || read back || [a class: (k_ca_nonzero, k_scan_lb), k_sel_rows] |
// [a threshold: k_sel_totals] | k_sel_samples | k_scan_lb | k_sel_nkeep | k_scan_lb x 2 | k_sel_alen | k_scan_lb | k_sel_ptrs |
// k_sel_gather_a | k_sel_gather_n || read back the sizes.
namespace {
constexpr u32 SEL_TPB = 256, SEL_ITEMS = 4;          // threads of the passes over the entries of A and N, and entries per thread (16-byte loads)
enum : int { SEL_ALL = 0, SEL_UNIQUE = 1, SEL_LOCUS_UNIQUE = 2, SEL_MULTI = 3 };
// thread j: column pointer j and entry j of N checked (ecb_count_alignments' contract)
__global__ __launch_bounds__(TPB) void k_sel_ncheck(const int* indptr_n, u32 n_samples, const int* indices_n, const int* data_n, u64 nnz_n, u32 n_ecs,
                                                    u64* words) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    const u32 err = ca_n_errors(j, indptr_n, n_samples, indices_n, data_n, nnz_n, n_ecs);
    if (err) atomicOr(reinterpret_cast<u32*>(words + 1), err);
}
// in_class[e] = 1 when row e is of the class asked for (SEL_ALL has no such array)
__global__ __launch_bounds__(TPB) void k_sel_rows(const int* indptr, u32 n_ecs, u64 nnz, const u32* bits_excl, const u32* nz_excl, int row_class,
                                                  u32* in_class) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e >= n_ecs) return;
    u32 pop, nzc;
    ca_row_counts(indptr, e, nnz, bits_excl, nz_excl, pop, nzc);
    in_class[e] = row_class == SEL_UNIQUE ? pop == 1u : row_class == SEL_LOCUS_UNIQUE ? nzc == 1u : nzc >= 2u;
}
// four consecutive entries of a CSR's or CSC's index and value arrays, by 16-byte loads where they are whole and aligned
__device__ __forceinline__ void sel_load4(const int* ix, const int* dx, u64 i0, u64 n, int* x, int* d) {
    if (i0 + SEL_ITEMS <= n && ((reinterpret_cast<uintptr_t>(ix) | reinterpret_cast<uintptr_t>(dx)) & 15u) == 0u) {
        const int4 q = reinterpret_cast<const int4*>(ix + i0)[0], r = reinterpret_cast<const int4*>(dx + i0)[0];
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w; d[0] = r.x; d[1] = r.y; d[2] = r.z; d[3] = r.w;
    } else {
#pragma unroll
        for (u32 j = 0; j < SEL_ITEMS; ++j) { x[j] = i0 + j < n ? ix[i0 + j] : 0; d[j] = i0 + j < n ? dx[i0 + j] : 0; }
    }
}
static_assert(SEL_ITEMS == 4, "sel_load4");
// thread t: entries [4t, 4t + 4) of N; totals[s] += the counts of column s over the rows in class.  A thread adds up within a column; a wave
// whose lanes all ended in one column (a column of 20 000 entries holds ~80 such waves) sends one add, other lanes their own.
__global__ __launch_bounds__(SEL_TPB) void k_sel_totals(const int* indptr_n, u32 n_samples, const int* indices_n, const int* data_n, u64 nnz_n,
                                                        const u32* in_class, u64* totals) {
    __shared__ u32 s_col[2];
    const u64 b0 = blockIdx.x * (u64)(SEL_TPB * SEL_ITEMS), b1 = std::min<u64>(nnz_n, b0 + SEL_TPB * SEL_ITEMS) - 1;
    ca_block_rows(indptr_n, n_samples, b0, b1, s_col);
    const u64 i0 = b0 + (u64)threadIdx.x * SEL_ITEMS;
    const u32 hi = s_col[1];
    u32 col = hi;                                    // (a thread beyond the end: nothing to add, to the last column)
    u64 acc = 0;
    if (i0 < nnz_n) {
        int e[SEL_ITEMS], c[SEL_ITEMS];
        sel_load4(indices_n, data_n, i0, nnz_n, e, c);
        col = ca_row_of(indptr_n, s_col[0], hi, i0);
#pragma unroll
        for (u32 j = 0; j < SEL_ITEMS; ++j) {
            const u64 i = i0 + j;
            if (i >= nnz_n) break;
            if (col < hi && (u64)(u32)indptr_n[col + 1] <= i) {
                if (acc) atomicAdd(reinterpret_cast<unsigned long long*>(totals + col), (unsigned long long)acc);
                acc = 0;
                col = ca_row_of(indptr_n, col + 1, hi, i);
            }
            if (c[j] > 0 && (!in_class || in_class[e[j]])) acc += (u64)c[j];
        }
    }
    const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)col);
    if (__all(col == first)) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
        if ((threadIdx.x & 63u) == 0u && acc) atomicAdd(reinterpret_cast<unsigned long long*>(totals + first), (unsigned long long)acc);
    } else if (acc) atomicAdd(reinterpret_cast<unsigned long long*>(totals + col), (unsigned long long)acc);
}
// sample s stays when it is named (named null: all are) and, with a threshold (totals not null), its total reaches it
__global__ __launch_bounds__(TPB) void k_sel_samples(u32 n_samples, const unsigned char* named, const u64* totals, u64 least, u32* skeep,
                                                     unsigned char* out_keep) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s >= n_samples) return;
    const bool k = (!named || named[s]) && (!totals || totals[s] >= least);
    skeep[s] = k;
    out_keep[s] = k;
}
// thread t: entries [4t, 4t + 4) of N; nkeep[j] = 1 when entry j stays (its row in class, its sample staying, its count above 0), and the row
// of such an entry is marked -- many entries write the same 1: plain stores
__global__ __launch_bounds__(SEL_TPB) void k_sel_nkeep(const int* indptr_n, u32 n_samples, const int* indices_n, const int* data_n, u64 nnz_n,
                                                       const u32* in_class, const u32* skeep, u32* nkeep, u32* row_kept) {
    __shared__ u32 s_col[2];
    const u64 b0 = blockIdx.x * (u64)(SEL_TPB * SEL_ITEMS), b1 = std::min<u64>(nnz_n, b0 + SEL_TPB * SEL_ITEMS) - 1;
    ca_block_rows(indptr_n, n_samples, b0, b1, s_col);
    const u64 i0 = b0 + (u64)threadIdx.x * SEL_ITEMS;
    if (i0 >= nnz_n) return;
    const u32 hi = s_col[1];
    int e[SEL_ITEMS], c[SEL_ITEMS];
    u32 k[SEL_ITEMS];
    sel_load4(indices_n, data_n, i0, nnz_n, e, c);
    u32 col = ca_row_of(indptr_n, s_col[0], hi, i0), stays = skeep[col];
#pragma unroll
    for (u32 j = 0; j < SEL_ITEMS; ++j) {
        const u64 i = i0 + j;
        k[j] = 0u;
        if (i >= nnz_n) continue;
        if (col < hi && (u64)(u32)indptr_n[col + 1] <= i) { col = ca_row_of(indptr_n, col + 1, hi, i); stays = skeep[col]; }
        if (stays && c[j] > 0 && (!in_class || in_class[e[j]])) { k[j] = 1u; row_kept[e[j]] = 1u; }
    }
    if (i0 + SEL_ITEMS <= nnz_n) reinterpret_cast<uint4*>(nkeep + i0)[0] = make_uint4(k[0], k[1], k[2], k[3]);
    else {
#pragma unroll
        for (u32 j = 0; j < SEL_ITEMS; ++j) if (i0 + j < nnz_n) nkeep[i0 + j] = k[j];
    }
}
// alen[e] = the length of row e when it stays, else 0: its scan is the new row pointers
__global__ __launch_bounds__(TPB) void k_sel_alen(const int* indptr, u32 n_ecs, const u32* row_kept, u32* alen) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e < n_ecs) alen[e] = row_kept[e] ? (u32)(indptr[e + 1] - indptr[e]) : 0u;
}
// thread t: the new row pointer of row t when it stays (and the last one, t = E); the new column pointer of sample t when it stays (and the
// last one, t = S) -- the place the scan over N's entries gives the first entry of its old column
__global__ __launch_bounds__(TPB) void k_sel_ptrs(u32 n_ecs, const u32* row_kept, const u32* newrow, const u32* apos, const int* indptr_n, u32 n_samples,
                                                  const u32* skeep, const u32* spos, const u32* npos, int* out_indptr_a, int* out_indptr_n) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t <= n_ecs && (t == n_ecs || row_kept[t])) out_indptr_a[newrow[t]] = (int)apos[t];
    if (t <= n_samples && (t == n_samples || skeep[t])) out_indptr_n[spos[t]] = (int)npos[indptr_n[t]];
}
// thread t: non-zeros [4t, 4t + 4) of A, read whole (16-byte loads however long the row), those of rows that stay written to their row's new
// place; four of one row that land on a 16-byte boundary go out as one store each
__global__ __launch_bounds__(SEL_TPB) void k_sel_gather_a(const int* indptr, u32 n_ecs, const int* indices, const int* data, u64 nnz, const u32* row_kept,
                                                         const u32* apos, int* out_indices, int* out_data) {
    __shared__ u32 s_row[2];
    const u64 b0 = blockIdx.x * (u64)(SEL_TPB * SEL_ITEMS), b1 = std::min<u64>(nnz, b0 + SEL_TPB * SEL_ITEMS) - 1;
    ca_block_rows(indptr, n_ecs, b0, b1, s_row);
    const u64 i0 = b0 + (u64)threadIdx.x * SEL_ITEMS;
    if (i0 >= nnz) return;
    const u32 hi = s_row[1];
    u32 r = ca_row_of(indptr, s_row[0], hi, i0);
    const bool whole = i0 + SEL_ITEMS <= nnz;
    const bool one = r == hi || (u64)(u32)indptr[r + 1] >= std::min<u64>(i0 + SEL_ITEMS, nnz);      // all of them in row r
    if (one && !row_kept[r]) return;
    int x[SEL_ITEMS], d[SEL_ITEMS];
    sel_load4(indices, data, i0, nnz, x, d);
    if (one && whole) {
        const u64 dst = (u64)apos[r] + (i0 - (u64)(u32)indptr[r]);
        if ((dst & 3u) == 0u && ((reinterpret_cast<uintptr_t>(out_indices) | reinterpret_cast<uintptr_t>(out_data)) & 15u) == 0u) {
            reinterpret_cast<int4*>(out_indices + dst)[0] = make_int4(x[0], x[1], x[2], x[3]);
            reinterpret_cast<int4*>(out_data + dst)[0] = make_int4(d[0], d[1], d[2], d[3]);
            return;
        }
    }
#pragma unroll
    for (u32 j = 0; j < SEL_ITEMS; ++j) {
        const u64 i = i0 + j;
        if (i >= nnz) break;
        if (r < hi && (u64)(u32)indptr[r + 1] <= i) r = ca_row_of(indptr, r + 1, hi, i);
        if (!row_kept[r]) continue;
        const u64 dst = (u64)apos[r] + (i - (u64)(u32)indptr[r]);
        out_indices[dst] = x[j];
        out_data[dst] = d[j];
    }
}
// thread t: entries [4t, 4t + 4) of N: one that stays goes to its new place with its row's new number (npos: nnz_n + 1 values)
__global__ __launch_bounds__(SEL_TPB) void k_sel_gather_n(const int* indices_n, const int* data_n, u64 nnz_n, const u32* npos, const u32* newrow,
                                                         int* out_indices_n, int* out_data_n) {
    const u64 i0 = (blockIdx.x * (u64)SEL_TPB + threadIdx.x) * SEL_ITEMS;
    if (i0 >= nnz_n) return;
    int e[SEL_ITEMS], c[SEL_ITEMS];
    sel_load4(indices_n, data_n, i0, nnz_n, e, c);
    u32 p = npos[i0];
#pragma unroll
    for (u32 j = 0; j < SEL_ITEMS; ++j) {
        if (i0 + j >= nnz_n) break;
        const u32 q = npos[i0 + j + 1];
        if (q != p) { out_indices_n[p] = (int)newrow[e[j]]; out_data_n[p] = c[j]; }
        p = q;
    }
}
int sel_check_args(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint64_t nnz_a, const void* indptr_a, const void* indices_a,
                   const void* data_a, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int32_t row_class,
                   const void* out_indptr_a, const void* out_indices_a, const void* out_data_a, const void* out_indptr_n, const void* out_indices_n,
                   const void* out_data_n, const void* out_sample_keep, const uint64_t* out_sizes) {
    RCCHK(ca_check_matrices(n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n));
    if (!out_indptr_a || !out_indptr_n || !out_sample_keep || !out_sizes || (nnz_a && (!out_indices_a || !out_data_a)) ||
        (nnz_n && (!out_indices_n || !out_data_n)))
        return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (row_class < SEL_ALL || row_class > SEL_MULTI) return fail(nullptr, ECB_ERR_ARG, "select: no such row class (%d)", (int)row_class);
    if (nnz_a >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "the matrices exceed the .bin format's int32 limits");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_select_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint64_t nnz_a, const void* d_indptr_a,
                                 const void* d_indices_a, const void* d_data_a, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                                 const void* d_data_n, int32_t row_class, const void* d_sample_keep, int64_t min_count, void* d_out_indptr_a,
                                 void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n, void* d_out_data_n,
                                 void* d_out_sample_keep, uint64_t* out_sizes) {
    RCCHK(sel_check_args(n_ecs, n_loci, n_haps, n_samples, nnz_a, d_indptr_a, d_indices_a, d_data_a, nnz_n, d_indptr_n, d_indices_n, d_data_n, row_class,
                         d_out_indptr_a, d_out_indices_a, d_out_data_a, d_out_indptr_n, d_out_indices_n, d_out_data_n, d_out_sample_keep, out_sizes));
    const u64 E = n_ecs, S = n_samples;
    const u64 pa = (E + 1) * 4, za = nnz_a * 4, pn = (S + 1) * 4, zn = nnz_n * 4;
    if (const SpanClash clash = span_clash({{d_indptr_a, pa}, {d_indices_a, za}, {d_data_a, za}, {d_indptr_n, pn}, {d_indices_n, zn}, {d_data_n, zn},
                                            {d_sample_keep, d_sample_keep ? S : 0}, {d_out_indptr_a, pa}, {d_out_indices_a, za}, {d_out_data_a, za},
                                            {d_out_indptr_n, pn}, {d_out_indices_n, zn}, {d_out_data_n, zn}, {d_out_sample_keep, S}}, 7))
        return fail(nullptr, ECB_ERR_ARG, "%s", clash == SPANS_OUT_IN ? "an output overlaps an input" : "the outputs overlap");
    Call c(device, "select: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const bool classed = row_class != SEL_ALL, threshold = min_count >= 0;
    // apply-mask's words: [0] the error bits of A, [1] of N, [2] [3] the totals of the classifier's scans, [4 .. 8) the sizes of the result
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);
    u64* words = c.get<u64>(n_words);
    u32* bits = c.get<u32>(nnz_a);
    u32 *bits_excl = classed ? c.get<u32>(nnz_a + 1) : nullptr, *in_class = classed ? c.get<u32>(E) : nullptr;
    u64* totals = threshold ? c.get<u64>(S) : nullptr;
    u32 *skeep = c.get<u32>(S), *spos = c.get<u32>(S + 1), *nkeep = c.get<u32>(nnz_n), *npos = c.get<u32>(nnz_n + 1);
    u32 *row_kept = c.get<u32>(E), *newrow = c.get<u32>(E + 1), *alen = c.get<u32>(E), *apos = c.get<u32>(E + 1);
    u32* sums = c.get<u32>(scan_words(std::max<u64>(std::max<u64>(nnz_a, nnz_n), std::max<u64>(E, S))));
    if (const int rc = c.missing()) return rc;
    const int *ipa = (const int*)d_indptr_a, *ixa = (const int*)d_indices_a, *daa = (const int*)d_data_a;
    const int *ipn = (const int*)d_indptr_n, *ixn = (const int*)d_indices_n, *dan = (const int*)d_data_n;
    CALLCHK(c, hipMemsetAsync(words, 0, n_words * 8, st));
    k_sel_ncheck<<<nblk(std::max<u64>(nnz_n, S + 1), TPB), TPB, 0, st>>>(ipn, n_samples, ixn, dan, nnz_n, n_ecs, words);
    k_gm_check<true><<<nblk(std::max<u64>(E + 1, (nnz_a + GM_ITEMS - 1) / GM_ITEMS), TPB), TPB, 0, st>>>(ipa, n_ecs, ixa, daa, nnz_a, nullptr, n_loci, n_haps,
                                                                                                       bits, words);
    CALLCHK(c, hipGetLastError());
    if (classed) CALLCHK(c, scan_launch(st, bits, nnz_a, bits_excl, sums, words + 3, 1, bits_excl + nnz_a));
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    if (classed && back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    // the input is well formed: from here on the outputs are written
    if (classed) {
        u32* nz_excl = nullptr;
        if ((u32)back[0] & GM_SAW_ZERO) {
            nz_excl = c.get<u32>(nnz_a + 1);
            if (const int rc = c.missing()) return rc;
            k_ca_nonzero<<<nblk(nnz_a, TPB), TPB, 0, st>>>(bits, nnz_a);      // (a stored 0 was seen: nnz_a > 0)
            CALLCHK(c, scan_launch(st, bits, nnz_a, nz_excl, sums, words + 2, 1, nz_excl + nnz_a));
        }
        if (E) k_sel_rows<<<nblk(E, TPB), TPB, 0, st>>>(ipa, n_ecs, nnz_a, bits_excl, nz_excl, row_class, in_class);
    }
    const unsigned n_blocks = nblk(nnz_n, SEL_TPB * SEL_ITEMS);
    if (threshold) {
        CALLCHK(c, hipMemsetAsync(totals, 0, S * 8, st));
        if (nnz_n) k_sel_totals<<<n_blocks, SEL_TPB, 0, st>>>(ipn, n_samples, ixn, dan, nnz_n, in_class, totals);
    }
    k_sel_samples<<<nblk(S, TPB), TPB, 0, st>>>(n_samples, (const unsigned char*)d_sample_keep, totals, (u64)std::max<int64_t>(min_count, 1), skeep,
                                               (unsigned char*)d_out_sample_keep);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, skeep, S, spos, sums, words + 6, 1, spos + S));
    CALLCHK(c, hipMemsetAsync(row_kept, 0, std::max<u64>(E, 1) * 4, st));
    if (nnz_n) k_sel_nkeep<<<n_blocks, SEL_TPB, 0, st>>>(ipn, n_samples, ixn, dan, nnz_n, in_class, skeep, nkeep, row_kept);
    CALLCHK(c, scan_launch(st, nkeep, nnz_n, npos, sums, words + 7, 1, npos + nnz_n));
    CALLCHK(c, scan_launch(st, row_kept, E, newrow, sums, words + 4, 1, newrow + E));
    if (E) k_sel_alen<<<nblk(E, TPB), TPB, 0, st>>>(ipa, n_ecs, row_kept, alen);
    CALLCHK(c, scan_launch(st, alen, E, apos, sums, words + 5, 1, apos + E));
    k_sel_ptrs<<<nblk(std::max<u64>(E, S) + 1, TPB), TPB, 0, st>>>(n_ecs, row_kept, newrow, apos, ipn, n_samples, skeep, spos, npos, (int*)d_out_indptr_a,
                                                             (int*)d_out_indptr_n);
    if (nnz_a) k_sel_gather_a<<<nblk(nnz_a, SEL_TPB * SEL_ITEMS), SEL_TPB, 0, st>>>(ipa, n_ecs, ixa, daa, nnz_a, row_kept, apos, (int*)d_out_indices_a,
                                                                                   (int*)d_out_data_a);
    if (nnz_n) k_sel_gather_n<<<n_blocks, SEL_TPB, 0, st>>>(ixn, dan, nnz_n, npos, newrow, (int*)d_out_indices_n, (int*)d_out_data_n);
    CALLCHK(c, hipGetLastError());
    u64 sizes[4];
    if (const int rc = c.read_back(sizes, words + 4, 4)) return rc;
    for (int k = 0; k < 4; ++k) out_sizes[k] = sizes[k];
    return ECB_OK;
}

extern "C" int ecb_select(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint64_t nnz_a, const int32_t* indptr_a,
                          const int32_t* indices_a, const int32_t* data_a, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
                          const int32_t* data_n, int32_t row_class, const uint8_t* sample_keep, int64_t min_count, int32_t* out_indptr_a,
                          int32_t* out_indices_a, int32_t* out_data_a, int32_t* out_indptr_n, int32_t* out_indices_n, int32_t* out_data_n,
                          uint8_t* out_sample_keep, uint64_t* out_sizes) {
    RCCHK(sel_check_args(n_ecs, n_loci, n_haps, n_samples, nnz_a, indptr_a, indices_a, data_a, nnz_n, indptr_n, indices_n, data_n, row_class,
                         out_indptr_a, out_indices_a, out_data_a, out_indptr_n, out_indices_n, out_data_n, out_sample_keep, out_sizes));
    Call c(device, "select: "); if (c.rc) return c.rc;
    const u64 rowb = ((u64)n_ecs + 1) * 4, colb = ((u64)n_samples + 1) * 4;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, sk, oia, oxa, oda, oin, oxn, odn, osk;
    std::vector<StageIn> in = {{&ipa, indptr_a, rowb}, {&ixa, indices_a, nnz_a * 4}, {&daa, data_a, nnz_a * 4}, {&ipn, indptr_n, colb},
                               {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4}, {&oia, nullptr, rowb}, {&oxa, nullptr, nnz_a * 4},
                               {&oda, nullptr, nnz_a * 4}, {&oin, nullptr, colb}, {&oxn, nullptr, nnz_n * 4}, {&odn, nullptr, nnz_n * 4},
                               {&osk, nullptr, n_samples}};
    if (sample_keep) in.push_back({&sk, sample_keep, n_samples});
    int rc = stage_in(c, in);
    uint64_t sizes[4] = {0, 0, 0, 0};
    if (rc == ECB_OK) rc = ecb_select_device(device, n_ecs, n_loci, n_haps, n_samples, nnz_a, ipa.p, ixa.p, daa.p, nnz_n, ipn.p, ixn.p, dan.p, row_class,
                                             sample_keep ? sk.p : nullptr, min_count, oia.p, oxa.p, oda.p, oin.p, oxn.p, odn.p, osk.p, sizes);
    RCCHK(rc);
    RCCHK(stage_out(c, {{out_indptr_a, &oia, (sizes[0] + 1) * 4}, {out_indices_a, &oxa, sizes[1] * 4}, {out_data_a, &oda, sizes[1] * 4},
                        {out_indptr_n, &oin, (sizes[2] + 1) * 4}, {out_indices_n, &oxn, sizes[3] * 4}, {out_data_n, &odn, sizes[3] * 4},
                        {out_sample_keep, &osk, n_samples}}));
    for (int k = 0; k < 4; ++k) out_sizes[k] = sizes[k];
    return ECB_OK;
}

// ---- ecmerge: several .bin files' A and N combined into one (ecb_combine / ecb_combine_device) ---------------------------------------------
// The rows of all parts are one concatenated index space: global row g = the part's first row + its own row, and g plays the "read" of the
// EC builder.  Every row becomes one Entry (hash, first_inv = ~g, its pairs in the merged column numbering, sorted) and k_merge puts them all
// into one table -- equal keys from one part or several find each other there exactly as two ranks' ECs do -- then ecb_finalize ranks the
// ECs by first appearance and emits CSR A.  A lookup pass gives every row its EC; N is the (output sample, EC) pairs of every part's N through
// the two maps, sorted, summed per pair, zeros dropped, written as CSC.  No loop over a row anywhere except the key compare of the lookup:
// the pair passes run one thread per non-zero, so rows of 1 and of 10 000 loci cost the same per pair.
// The empty key (a row without pairs) is a key like any other: n = 0, hash finish_hash(0, 0) = 1, n1 = 1 in its slot; ListCmp compares
// zero pairs and finds it equal, k_merge stores nothing and publishes n1, and the emit writes a row of length 0.
namespace {
struct CbPart {                                  // one part, device pointers, and where it sits in the concatenation
    const int *ipa, *ixa, *daa, *ipn, *ixn, *dan;
    const u32 *tmap, *smap;
    u32 n_ecs, n_loci, n_samples, pad;
    u64 nnz_a, nnz_n;
};
// base arrays (u64, n_parts + 1 each, exclusive sums): rows, pairs, N non-zeros, row pointers (E + 1 per part), N column pointers (S + 1)
enum { CB_ROWS = 0, CB_PAIRS, CB_NZ, CB_APTR, CB_NPTR, CB_BASES };
enum : u32 { CB_ERR_PTR = 1u, CB_ERR_LOCUS = 2u, CB_ERR_BITS = 4u, CB_ERR_ORDER = 8u, CB_ERR_MAP = 16u, CB_ERR_NPTR = 32u, CB_ERR_NEC = 64u,
             CB_ERR_NCOUNT = 128u, CB_ERR_SMAP = 256u, CB_ERR_LOST = 512u, CB_ERR_SUM = 1024u,
             BD_ERR_MPTR = 2048u, BD_ERR_MIDX = 4096u, BD_ERR_MORDER = 8192u, BD_ERR_WIDE = 16384u };      // (ecb_bundle's group map)
constexpr u32 CB_SHARDS = 256, CB_SHARD_WORDS = 16;    // arena sizing: per shard (its own 128-byte line) the largest and the summed wave demand
// the largest p < n with base[p] <= x (x below base[n]: an empty part never wins, the part after it starts at the same place)
__device__ __forceinline__ u32 cb_find(const u64* base, u32 n, u64 x) {
    u32 a = 0, b = n;
    while (b - a > 1) { const u32 m = (a + b) >> 1; if (base[m] <= x) a = m; else b = m; }
    return a;
}
// the row of non-zero i of a CSR whose row pointers have been checked: the largest e < E with ptr[e] <= i
__device__ __forceinline__ u32 cb_row(const int* ptr, u32 E, long long i) {
    u32 a = 0, b = E;
    while (b - a > 1) { const u32 m = (a + b) >> 1; if ((long long)ptr[m] <= i) a = m; else b = m; }
    return a;
}
// inclusive sum of v over the lanes of a run of equal keys (keys non-decreasing over the wave's lanes; the lanes past the end come last and
// never feed a valid lane).  Written by the run's last lane: a plain store when the run lies inside the wave, an add when it goes on in a
// neighbouring wave (dst zeroed) -- one write per run, not one atomic per element.
__device__ __forceinline__ void cb_run_sum(u64 key, u64 v, bool valid, u64 i, u64 n, const u64* keys, u64* dst, u64 at) {
    const u32 lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 ov = __shfl_up(v, d), ok = __shfl_up(key, d);
        if ((int)lane >= d && ok == key) v += ov;
    }
    const u64 nk = __shfl_down(key, 1);
    const bool nvalid = __shfl_down((int)valid, 1) != 0;
    const u64 k0 = __shfl(key, 0);
    if (!valid) return;
    if (lane != 63u && nvalid && nk == key) return;                     // not the run's last lane in this wave
    const u64 i0 = i - lane;                                             // the wave's first element
    const bool before = key == k0 && i0 > 0 && keys[i0 - 1] == key;
    const bool after = i + 1 < n && keys[i + 1] == key;                  // (only the wave's last lane can see its run go on)
    if (before || after) atomicAdd(reinterpret_cast<unsigned long long*>(dst + at), (unsigned long long)v);
    else dst[at] = v;
}
// pointer k of the n + 1 of a CSR / CSC with nnz entries: from 0 to nnz, never falling
__device__ __forceinline__ bool cb_ptr_bad(const int* ptr, u64 k, u64 n, u64 nnz) {
    const long long a = ptr[k];
    if (a < 0 || (u64)a > nnz || (k == 0 && a != 0) || (k == n && (u64)a != nnz)) return true;
    return k < n && ptr[k + 1] < a;
}
// non-zero li of row r of a part's A (checked pointers): its mask, its column, its place after the one before it
__device__ __forceinline__ u32 cb_nz_bad(const CbPart& q, long long li, u32 r, u32 n_haps, int c, u32 d) {
    u32 e = 0;
    if (d == 0u || (d >> n_haps) != 0u) e |= CB_ERR_BITS;
    if (c < 0 || (u32)c >= q.n_loci) e |= CB_ERR_LOCUS;
    if (li > q.ipa[r] && q.ixa[li - 1] >= c) e |= CB_ERR_ORDER;                          // ascending as the part stores it
    return e;
}
// the error bits of a wave's lanes into the call's error word: one atomic per wave that has any
__device__ __forceinline__ void cb_raise(u32 e, u32* err) {
    if (__ballot(e != 0u)) {
        u32 w = e;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) w |= (u32)__shfl_xor((int)w, d);
        if ((threadIdx.x & 63u) == 0u) atomicOr(err, w);
    }
}
// row pointers of A (one thread per pointer of every part) and column pointers of N
__global__ __launch_bounds__(TPB) void k_cb_check(const CbPart* P, u32 n_parts, const u64* base, u32* err) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    const u64* ab = base + CB_APTR * (n_parts + 1);
    const u64* nb = base + CB_NPTR * (n_parts + 1);
    u32 e = 0;
    if (t < ab[n_parts]) {
        const u32 p = cb_find(ab, n_parts, t);
        const CbPart& q = P[p];
        const u64 k = t - ab[p];
        if (cb_ptr_bad(q.ipa, k, q.n_ecs, q.nnz_a)) e |= CB_ERR_PTR;
    }
    if (t < nb[n_parts]) {
        const u32 p = cb_find(nb, n_parts, t);
        const CbPart& q = P[p];
        const u64 k = t - nb[p];
        if (cb_ptr_bad(q.ipn, k, q.n_samples, q.nnz_n)) e |= CB_ERR_NPTR;
    }
    if (__ballot(e != 0u)) {
        u32 w = e;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) w |= (u32)__shfl_xor((int)w, d);
        if ((threadIdx.x & 63u) == 0u) atomicOr(err, w);
    }
}
// one thread per non-zero of every part: checked, its column mapped, out as (global row << 32 | merged column, mask) -- the sort key
__global__ __launch_bounds__(TPB) void k_cb_pairs(const CbPart* P, u32 n_parts, const u64* base, u32 n_loci, u32 n_haps, u64* keys, u32* vals, u32* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const u64* pb = base + CB_PAIRS * (n_parts + 1);
    u32 e = 0;
    if (i < pb[n_parts]) {
        const u32 p = cb_find(pb, n_parts, i);
        const CbPart& q = P[p];
        const long long li = (long long)(i - pb[p]);
        const u32 r = cb_row(q.ipa, q.n_ecs, li);
        const int c = q.ixa[li];
        const u32 d = (u32)q.daa[li];
        u32 m = 0;
        e = cb_nz_bad(q, li, r, n_haps, c, d);
        if (!(e & CB_ERR_LOCUS)) {
            m = q.tmap ? q.tmap[c] : (u32)c;
            if (m >= n_loci) e |= CB_ERR_MAP;
        }
        keys[i] = ((base[CB_ROWS * (n_parts + 1) + p] + r) << 32) | m;
        vals[i] = d;
    }
    if (__ballot(e != 0u)) {
        u32 w = e;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) w |= (u32)__shfl_xor((int)w, d);
        if ((threadIdx.x & 63u) == 0u) atomicOr(err, w);
    }
}
// the pairs in (row, column) order -> the key list k_merge reads, and every row's set hash (sum of pair_hash64 over its pairs); a column
// that repeats within a row (a target map that sends two columns to one) is refused here
__global__ __launch_bounds__(TPB) void k_cb_hash(const u64* keys, const u32* vals, u64 n, uint2* pairs, u64* rowhash, u32* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const bool valid = i < n;
    u64 k = ~0ull, h = 0, row = 0;
    bool dup = false;
    if (valid) {
        k = keys[i];
        row = k >> 32;
        const u32 col = (u32)k, mask = vals[i];
        pairs[i] = make_uint2(col, mask);
        h = pair_hash64(col, mask);
        dup = i > 0 && (keys[i - 1] >> 32) == row && keys[i - 1] >= k;
    }
    if (__ballot(dup) && (threadIdx.x & 63u) == 0u) atomicOr(err, CB_ERR_ORDER);
    // (runs are rows: the row is the key's high word, and a row's pairs are adjacent)
    const u64 rk = valid ? row : ~0ull;
    const u32 lane = threadIdx.x & 63u;
    u64 v = h;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 ov = __shfl_up(v, d), ok = __shfl_up(rk, d);
        if ((int)lane >= d && ok == rk) v += ov;
    }
    const u64 nk = __shfl_down(rk, 1), k0 = __shfl(rk, 0);
    if (!valid || (lane != 63u && nk == rk)) return;
    const u64 i0 = i - lane;
    const bool before = rk == k0 && i0 > 0 && (keys[i0 - 1] >> 32) == rk;
    const bool after = i + 1 < n && (keys[i + 1] >> 32) == rk;
    if (before || after) atomicAdd(reinterpret_cast<unsigned long long*>(rowhash + row), (unsigned long long)v);
    else rowhash[row] = v;
}
// one Entry per global row (k_merge's exchange format), and per aligned 64 rows -- one k_merge wave -- the arena pairs it reserves
// (rowptr: the global rows' places in the pair list when it is not the parts' own pairs one after the other -- ecb_bundle's folded rows)
__global__ __launch_bounds__(TPB) void k_cb_entries(const CbPart* P, u32 n_parts, const u64* base, const u32* rowptr, const u64* rowhash, Entry* ent,
                                                    u64* words) {
    const u64 g = blockIdx.x * (u64)TPB + threadIdx.x;
    const u64* rb = base + CB_ROWS * (n_parts + 1);
    u32 over = 0;
    if (g < rb[n_parts]) {
        u32 off, n;
        if (rowptr) { off = rowptr[g]; n = rowptr[g + 1] - off; }
        else {
            const u32 p = cb_find(rb, n_parts, g);
            const CbPart& q = P[p];
            const u64 r = g - rb[p];
            const u32 a = (u32)q.ipa[r];
            n = (u32)q.ipa[r + 1] - a;
            off = (u32)(base[CB_PAIRS * (n_parts + 1) + p] + a);
        }
        Entry en;
        en.lo = finish_hash(rowhash[g], n); en.reserved = 0; en.count = 0; en.first_inv = ~(u32)g;
        en.off = off; en.n = n;
        ent[g] = en;
        over = n > INL ? n - INL : 0u;
    }
    const u32 ws = wave_sum(over);
    if ((threadIdx.x & 63u) == 0u && ws) {
        u64* s = words + CB_SHARD_WORDS * (1 + (g >> 6) % CB_SHARDS);
        atomicMax(reinterpret_cast<unsigned long long*>(s), (unsigned long long)ws);
        atomicAdd(reinterpret_cast<unsigned long long*>(s + 1), (unsigned long long)ws);
    }
}
// every row's EC: its hash, then its key compared pair for pair with the slot's (both in column order, as k_merge stored them); no slot
// is created.  A row that finds no slot is an internal error (CB_ERR_LOST).
__global__ __launch_bounds__(TPB) void k_cb_lookup(const Entry* ent, u64 n, const uint2* pairs, const Slot* table, u64 cap_mask, const uint2* arena,
                                                   const u32* rank_of_slot, u32* ec_of_row, u32* err) {
    const u64 g = blockIdx.x * (u64)TPB + threadIdx.x;
    if (g >= n) return;
    const Entry en = ent[g];
    u64 j = en.lo & cap_mask;
    for (u64 probe = 0; probe <= cap_mask; ++probe, j = (j + 1) & cap_mask) {
        const Slot& s = table[j];
        if (s.lo == 0ull) break;
        if (s.lo != en.lo || s.n1 != en.n + 1u) continue;
        bool same = true;
        for (u32 t = 0; t < en.n && same; ++t) {
            const uint2 a = key_pair(s, arena, t), b = pairs[(u64)en.off + t];
            same = a.x == b.x && a.y == b.y;
        }
        if (same) { ec_of_row[g] = rank_of_slot[j]; return; }
    }
    ec_of_row[g] = 0;
    atomicOr(err, CB_ERR_LOST);
}
// one thread per non-zero of every part's N: (output sample << 32 | EC, count)
__global__ __launch_bounds__(TPB) void k_cb_ntrip(const CbPart* P, u32 n_parts, const u64* base, u32 n_samples, const u32* ec_of_row,
                                                  u64* keys, u32* vals, u32* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const u64* zb = base + CB_NZ * (n_parts + 1);
    u32 e = 0;
    if (i < zb[n_parts]) {
        const u32 p = cb_find(zb, n_parts, i);
        const CbPart& q = P[p];
        const long long li = (long long)(i - zb[p]);
        const u32 s = cb_row(q.ipn, q.n_samples, li);
        const int r = q.ixn[li], c = q.dan[li];
        const u32 os = q.smap ? q.smap[s] : s;
        u32 ec = 0;
        if (r < 0 || (u32)r >= q.n_ecs) e |= CB_ERR_NEC;
        else ec = ec_of_row[base[CB_ROWS * (n_parts + 1) + p] + (u32)r];
        if (c < 0) e |= CB_ERR_NCOUNT;
        if (os >= n_samples) e |= CB_ERR_SMAP;
        keys[i] = ((u64)os << 32) | ec;
        vals[i] = c < 0 ? 0u : (u32)c;
    }
    if (__ballot(e != 0u)) {
        u32 w = e;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) w |= (u32)__shfl_xor((int)w, d);
        if ((threadIdx.x & 63u) == 0u) atomicOr(err, w);
    }
}
// sorted (sample, EC) keys -> one sum per distinct key (run id = exclusive scan of the head flags), and each run's key
__global__ __launch_bounds__(TPB) void k_cb_nsum(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u64* sums, u64* runkey) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const bool valid = i < n;
    u64 k = ~0ull, v = 0, at = 0;
    if (valid) {
        k = keys[i]; v = vals[i];
        at = pos[i] + flag[i] - 1u;
        if (flag[i]) runkey[at] = k;
    }
    cb_run_sum(k, v, valid, i, n, keys, sums, at);
}
// (every one of the n flags is written -- the scan behind reads them all -- and the run count is bounded by n whatever the device holds)
__global__ void k_cb_nkeep(const u64* sums, const u64* n_runs, u64 n, u32* keep, u32* err) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u64 s = r < min(*n_runs, n) ? sums[r] : 0ull;
    keep[r] = s != 0ull;
    if (s > (u64)INT_MAX) atomicOr(err, CB_ERR_SUM);
}
__global__ void k_cb_nemit(const u64* sums, const u64* runkey, const u32* keep, const u32* opos, const u64* n_runs, u64 n, int* indices, int* data, u64* okey) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r >= min(*n_runs, n) || !keep[r]) return;
    const u32 o = opos[r];
    indices[o] = (int)(u32)runkey[r];
    data[o] = (int)sums[r];
    okey[o] = runkey[r];
}
// column pointers of the output N: column s starts at the first kept key of sample s
__global__ void k_cb_nptr(const u64* okey, const u64* n_out, u64 n, u32 n_samples, int* indptr) {
    const u64 s = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (s <= n_samples) indptr[s] = (int)lower_bound_u64(okey, min(*n_out, n), s << 32);
}
const ErrBit CB_ERRS[] = {
    {CB_ERR_PTR, ECB_ERR_CONTRACT, "malformed CSR A: row pointers do not start at 0, go backwards or do not end at nnz"},
    {CB_ERR_NPTR, ECB_ERR_CONTRACT, "malformed CSC N: column pointers do not start at 0, go backwards or do not end at nnz"},
    {CB_ERR_LOCUS, ECB_ERR_CONTRACT, "malformed CSR A: a column at or beyond the part's n_loci"},
    {CB_ERR_BITS, ECB_ERR_CONTRACT, "malformed CSR A: a stored 0 or a haplotype bit at or beyond n_haplotypes"},
    {CB_ERR_MAP, ECB_ERR_CONTRACT, "a target map sends a column at or beyond n_loci"},
    {CB_ERR_ORDER, ECB_ERR_CONTRACT, "malformed CSR A: columns not strictly ascending within a row (unsorted or duplicate, before or after the target map)"},
    {CB_ERR_NEC, ECB_ERR_CONTRACT, "malformed CSC N: an EC index at or beyond the part's n_ecs"},
    {CB_ERR_NCOUNT, ECB_ERR_CONTRACT, "malformed CSC N: a negative count"},
    {CB_ERR_SMAP, ECB_ERR_CONTRACT, "a sample map sends a sample at or beyond n_samples"},
    {CB_ERR_SUM, ECB_ERR_LIMIT, "a merged count exceeds int32"},
    {BD_ERR_MPTR, ECB_ERR_CONTRACT, "malformed group map: pointers do not start at 0, go backwards or do not end at the number of group ids"},
    {BD_ERR_MIDX, ECB_ERR_CONTRACT, "malformed group map: a group id at or beyond n_groups"},
    {BD_ERR_MORDER, ECB_ERR_CONTRACT, "malformed group map: group ids not strictly ascending within a locus (unsorted or duplicate)"},
    {BD_ERR_WIDE, ECB_ERR_LIMIT, "group map: a locus in more than 65535 groups"},
    {CB_ERR_LOST, ECB_ERR_HIP, "internal: a row found no EC"},
};
struct HandleGuard { std::vector<ecb_handle*> h; ~HandleGuard() { for (ecb_handle* x : h) ecb_destroy(x); } };
// What ecb_combine and ecb_bundle hand to the steps they share (cb_finish): the rows of all parts as one index space, their pairs as
// sorted (row << 32 | column, mask) keys, and the scratch both sides use.
constexpr u64 CB_WORDS = CB_SHARD_WORDS * (1 + CB_SHARDS);     // status words: [0] error bits (u32), then the arena shards
struct CbRun {
    u32 n_parts, n_loci, n_haps, n_samples;          // (n_loci: the output's columns)
    u64 R, NP, NZ;                                   // rows, pairs in `keys`, N non-zeros of all parts
    const CbPart* d_parts; const u64* d_base;
    u64* words;
    u64 *keys0, *keys1; u32 *vals0, *vals1;          // sort buffers of max(NP, NZ): free for N once the pairs have been read
    const u64* keys; const u32* vals;                // the NP pairs in (row, column) order
    const u32* rowptr;                               // R + 1 places of the rows in them, or null: the parts' own row pointers
    u64* rowhash; uint2* pairs; Entry* ent;          // R zeroed, NP, R
    u32* err() const { return reinterpret_cast<u32*>(words); }
};
// one wait: the error word (refused by CB_ERRS) and the shards
int cb_refusal(Call& c, const CbRun& w, u64* back = nullptr) {
    std::vector<u64> own(back ? 0 : CB_WORDS);
    return c.read_back(back ? back : own.data(), w.words, CB_WORDS, CB_ERRS);
}
// steps 4-8 of the merge: key lists and row hashes, entries, one table, its ECs ranked and exported as A, every row's EC, N
int cb_finish(Call& c, const CbRun& w, void* d_out_indptr_a, void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n,
              void* d_out_data_n, uint64_t* out_sizes) {
    hipStream_t& st = c.st;                              // (the handle's own stream once there is one: it queues the slot ranks)
    const u32 n_parts = w.n_parts, n_samples = w.n_samples;
    const u64 R = w.R, NP = w.NP, NZ = w.NZ;
    u32* err = w.err();
    std::vector<u64> back(CB_WORDS);
    auto check = [&] { return cb_refusal(c, w, back.data()); };
    // 4. key lists and row hashes; 5. the entries, and the key arena's worst wave
    if (NP) k_cb_hash<<<nblk(NP, TPB), TPB, 0, st>>>(w.keys, w.vals, NP, w.pairs, w.rowhash, err);
    if (R) k_cb_entries<<<nblk(R, TPB), TPB, 0, st>>>(w.d_parts, n_parts, w.d_base, w.rowptr, w.rowhash, w.ent, w.words);
    RCCHK(check());
    u64 wmax = 0, wsum = 0;
    for (u32 k = 1; k <= CB_SHARDS; ++k) { wmax = std::max<u64>(wmax, back[CB_SHARD_WORDS * k]); wsum += back[CB_SHARD_WORDS * k + 1]; }
    u64 E = 0, nnz_a = 0, nnz_n = 0;
    u32* ec_of_row = c.get<u32>(R);                      // EC of every global row
    RCCHK(c.missing());
    HandleGuard hg;
    if (R) {
        // 6. one table: room for every row being an EC of its own (half full at most: no growth), and a key arena in which every wave's one
        //    reservation fits one of its 64 regions whatever the others took (arena_alloc: a region that cannot take a reservation is skipped)
        ecb_config cfg{};
        cfg.struct_size = sizeof(ecb_config); cfg.device = c.device; cfg.n_loci = w.n_loci; cfg.n_haplotypes = w.n_haps;
        cfg.ec_capacity = 2 * R;
        cfg.arena_capacity = std::max<u64>(1ull << 22, (u64)ARENA_REGIONS * (wmax + wsum / ARENA_REGIONS + 2));
        ecb_handle* h = nullptr;
        RCCHK(ecb_create(&cfg, &h));
        hg.h.push_back(h);
        ecb_add_counters(h, 0, R, R);                     // R "reads", all valid: the ranking's bitmap spans the rows
        int rc = ecb_table_merge_device(h, w.ent, R, w.pairs, NP);
        ecb_sizes sz{};
        if (rc == ECB_OK) rc = ecb_finalize(h, &sz);
        if (rc == ECB_OK) rc = ecb_export_device(h, d_out_indptr_a, d_out_indices_a, d_out_data_a, nullptr, nullptr, nullptr);
        if (rc == ECB_OK) rc = ensure_slot_ranks(h, sz.n_ecs);
        if (rc != ECB_OK) return fail(nullptr, rc, "%s%s", c.prefix, h->err.c_str());
        E = sz.n_ecs; nnz_a = sz.nnz_a;
        st = h->stream;
        // 7. every row's EC
        k_cb_lookup<<<nblk(R, TPB), TPB, 0, st>>>(w.ent, R, w.pairs, h->table, h->cap - 1, h->arena, h->run.csr.rank_of_slot, ec_of_row, err);
    } else {
        CALLCHK(c, hipMemsetAsync(d_out_indptr_a, 0, 4, st));
    }
    // 8. N: (sample, EC) keys sorted, summed per key, zeros dropped, CSC
    if (NZ) {
        u32 *flag = c.get<u32>(NZ), *pos = c.get<u32>(NZ + 1), *keep = c.get<u32>(NZ), *opos = c.get<u32>(NZ + 1);
        u32 *sums1 = c.get<u32>(scan_words(NZ)), *sums2 = c.get<u32>(scan_words(NZ));
        u64 *rsum = c.get<u64>(NZ), *rkey = c.get<u64>(NZ), *okey = c.get<u64>(NZ), *tot = c.get<u64>(2);
        SortScratch sc{c.get<u32>(rs_words(NZ)), c.get<u32>(RS_AUX_WORDS), w.words + 1};
        RCCHK(c.missing());
        k_cb_ntrip<<<nblk(NZ, TPB), TPB, 0, st>>>(w.d_parts, n_parts, w.d_base, n_samples, ec_of_row, w.keys0, w.vals0, err);
        RCCHK(check());
        SortBufs s{{w.keys0, w.keys1}, {w.vals0, w.vals1}};
        CALLCHK(c, radix_sort_pairs64(st, s, NZ, sc, msb_mask(((u64)n_samples - 1) << 32 | (E ? E - 1 : 0))));
        const u64* sk = s.keys(); const u32* sv = s.vals();
        CALLCHK(c, hipMemsetAsync(rsum, 0, NZ * 8, st));
        CALLCHK(c, hipMemsetAsync(tot, 0, 16, st));
        k_run_heads<<<nblk(NZ, TPB), TPB, 0, st>>>(sk, NZ, flag);
        CALLCHK(c, scan_launch(st, flag, NZ, pos, sums1, tot));
        k_cb_nsum<<<nblk(NZ, TPB), TPB, 0, st>>>(sk, sv, flag, pos, NZ, rsum, rkey);
        k_cb_nkeep<<<nblk(NZ, TPB), TPB, 0, st>>>(rsum, tot, NZ, keep, err);
        CALLCHK(c, scan_launch(st, keep, NZ, opos, sums2, tot + 1));
        k_cb_nemit<<<nblk(NZ, TPB), TPB, 0, st>>>(rsum, rkey, keep, opos, tot, NZ, (int*)d_out_indices_n, (int*)d_out_data_n, okey);
        k_cb_nptr<<<nblk((u64)n_samples + 1, TPB), TPB, 0, st>>>(okey, tot + 1, NZ, n_samples, (int*)d_out_indptr_n);
        u64 t2[2] = {0, 0};
        CALLCHK(c, hipMemcpyAsync(t2, tot, 16, hipMemcpyDeviceToHost, st));
        RCCHK(check());
        if (t2[1] > NZ) return fail(nullptr, ECB_ERR_HIP, "internal: %llu N entries from %llu", (unsigned long long)t2[1], (unsigned long long)NZ);
        nnz_n = t2[1];
    } else {
        CALLCHK(c, hipMemsetAsync(d_out_indptr_n, 0, ((u64)n_samples + 1) * 4, st));
        RCCHK(check());
    }
    out_sizes[0] = E; out_sizes[1] = nnz_a; out_sizes[2] = nnz_n;
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_combine_device(int device, uint32_t n_parts, const ecb_combine_part* parts, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples,
                                  void* d_out_indptr_a, void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n,
                                  void* d_out_data_n, uint64_t* out_sizes) {
    if (!parts || !n_parts || !out_sizes || !d_out_indptr_a || !d_out_indptr_n || !n_loci || !n_haps || n_haps > 31)
        return fail(nullptr, ECB_ERR_ARG, "combine: bad argument");
    if (n_loci >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "combine: n_loci out of range (1 .. 2^26-3)");
    const u32 B = n_parts + 1;
    std::vector<u64> base((u64)CB_BASES * B, 0);
    std::vector<CbPart> hp(n_parts);
    for (u32 p = 0; p < n_parts; ++p) {
        const ecb_combine_part& c = parts[p];
        if (c.struct_size != sizeof(ecb_combine_part)) return fail(nullptr, ECB_ERR_ARG, "combine: part %u: bad struct_size", p);
        if (!c.indptr_a || !c.indptr_n || (c.nnz_a && (!c.indices_a || !c.data_a)) || (c.nnz_n && (!c.indices_n || !c.data_n)))
            return fail(nullptr, ECB_ERR_ARG, "combine: part %u: null array", p);
        if (c.n_samples && !c.sample_map) return fail(nullptr, ECB_ERR_ARG, "combine: part %u: no sample map", p);
        if (!c.target_map && c.n_loci != n_loci) return fail(nullptr, ECB_ERR_ARG, "combine: part %u: no target map, but %u loci against %u", p, c.n_loci, n_loci);
        if (c.nnz_a >= (1ull << 31) || c.nnz_n >= (1ull << 31) || c.n_ecs >= (1u << 31) - 1u || c.n_samples >= (1u << 31) - 1u)
            return fail(nullptr, ECB_ERR_LIMIT, "combine: part %u exceeds the .bin format's int32 limits", p);
        hp[p] = CbPart{(const int*)c.indptr_a, (const int*)c.indices_a, (const int*)c.data_a, (const int*)c.indptr_n, (const int*)c.indices_n,
                       (const int*)c.data_n, c.target_map, c.sample_map, c.n_ecs, c.n_loci, c.n_samples, 0u, c.nnz_a, c.nnz_n};
        const u64 add[CB_BASES] = {c.n_ecs, c.nnz_a, c.nnz_n, (u64)c.n_ecs + 1, (u64)c.n_samples + 1};
        for (int k = 0; k < CB_BASES; ++k) base[(u64)k * B + p + 1] = base[(u64)k * B + p] + add[k];
    }
    const u64 R = base[CB_ROWS * B + n_parts], NP = base[CB_PAIRS * B + n_parts], NZ = base[CB_NZ * B + n_parts];
    // (the outputs are bounded by these sums, which is what the caller allocates; the sort of N takes fewer than 2^30 keys)
    if (R >= (1ull << 31) - 1 || NP >= (1ull << 31) || NZ >= (1ull << 30) || n_samples >= (1u << 31) - 1u)
        return fail(nullptr, ECB_ERR_LIMIT, "combine: the merged sizes exceed the .bin format's int32 limits");
    if ((R && (!d_out_indices_a || !d_out_data_a)) || (NZ && (!d_out_indices_n || !d_out_data_n))) return fail(nullptr, ECB_ERR_ARG, "combine: null output");
    bool any_map = false;
    for (u32 p = 0; p < n_parts; ++p) any_map |= hp[p].tmap != nullptr;
    if (any_map && NP >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "combine: more than 2^30 non-zeros to re-sort after a target map");
    Call c(device, "combine: ", true); if (c.rc) return c.rc;
    hipStream_t& st = c.st;
    CbRun w{};
    w.n_parts = n_parts; w.n_loci = n_loci; w.n_haps = n_haps; w.n_samples = n_samples; w.R = R; w.NP = NP; w.NZ = NZ;
    CbPart* d_parts = c.get<CbPart>(n_parts);
    u64* d_base = c.get<u64>(base.size());
    w.d_parts = d_parts; w.d_base = d_base;
    w.words = c.get<u64>(CB_WORDS);
    const u64 NK = std::max(NP, NZ);                     // (the sort buffers serve the pairs of A, then the entries of N)
    w.keys0 = c.get<u64>(NK); w.keys1 = c.get<u64>(NK); w.rowhash = c.get<u64>(R);
    w.vals0 = c.get<u32>(NK); w.vals1 = c.get<u32>(NK);
    w.pairs = c.get<uint2>(NP);
    w.ent = c.get<Entry>(R);
    RCCHK(c.missing());
    CALLCHK(c, hipMemcpyAsync(d_parts, hp.data(), n_parts * sizeof(CbPart), hipMemcpyHostToDevice, st));
    CALLCHK(c, hipMemcpyAsync(d_base, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
    CALLCHK(c, hipMemsetAsync(w.words, 0, CB_WORDS * 8, st));
    CALLCHK(c, hipMemsetAsync(w.rowhash, 0, std::max<u64>(R, 1) * 8, st));
    // 1. the pointers; 2. the pairs (their binary searches trust checked pointers)
    const u64 n_ptr = std::max(base[CB_APTR * B + n_parts], base[CB_NPTR * B + n_parts]);
    k_cb_check<<<nblk(n_ptr, TPB), TPB, 0, st>>>(d_parts, n_parts, d_base, w.err());
    RCCHK(cb_refusal(c, w));
    if (NP) k_cb_pairs<<<nblk(NP, TPB), TPB, 0, st>>>(d_parts, n_parts, d_base, n_loci, n_haps, w.keys0, w.vals0, w.err());
    RCCHK(cb_refusal(c, w));
    // 3. rows that a target map re-numbered are re-sorted: one radix sort of (row, column) over all pairs (parts without a map are sorted already)
    w.keys = w.keys0; w.vals = w.vals0;
    if (any_map && NP > 1) {
        SortScratch sc{c.get<u32>(rs_words(NP)), c.get<u32>(RS_AUX_WORDS), w.words + 1};
        RCCHK(c.missing());
        SortBufs s{{w.keys0, w.keys1}, {w.vals0, w.vals1}};
        CALLCHK(c, radix_sort_pairs64(st, s, NP, sc, msb_mask((R - 1) << 32 | (n_loci - 1))));
        w.keys = s.keys(); w.vals = s.vals();
    }
    return cb_finish(c, w, d_out_indptr_a, d_out_indices_a, d_out_data_a, d_out_indptr_n, d_out_indices_n, d_out_data_n, out_sizes);
}

extern "C" int ecb_combine(int device, uint32_t n_parts, const ecb_combine_part* parts, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples,
                           int32_t* out_indptr_a, int32_t* out_indices_a, int32_t* out_data_a, int32_t* out_indptr_n, int32_t* out_indices_n,
                           int32_t* out_data_n, uint64_t* out_sizes) {
    if (!parts || !n_parts || !out_sizes || !out_indptr_a || !out_indptr_n) return fail(nullptr, ECB_ERR_ARG, "combine: bad argument");
    Call c(device, "combine: "); if (c.rc) return c.rc;
    std::vector<ecb_combine_part> dp(parts, parts + n_parts);
    std::vector<DevBuf<>> bufs((u64)n_parts * 8);
    std::vector<StageIn> in;
    std::vector<const void**> at;                        // (the pointer of dp that each staged array replaces)
    u64 R = 0, NP = 0, NZ = 0;
    for (u32 p = 0; p < n_parts; ++p) {
        const ecb_combine_part& c = parts[p];
        if (c.struct_size != sizeof(ecb_combine_part)) return fail(nullptr, ECB_ERR_ARG, "combine: part %u: bad struct_size", p);
        const void* src[8] = {c.indptr_a, c.indices_a, c.data_a, c.indptr_n, c.indices_n, c.data_n, c.target_map, c.sample_map};
        const u64 len[8] = {((u64)c.n_ecs + 1) * 4, c.nnz_a * 4, c.nnz_a * 4, ((u64)c.n_samples + 1) * 4, c.nnz_n * 4, c.nnz_n * 4, (u64)c.n_loci * 4, (u64)c.n_samples * 4};
        const void** dst[8] = {(const void**)&dp[p].indptr_a, (const void**)&dp[p].indices_a, (const void**)&dp[p].data_a, (const void**)&dp[p].indptr_n,
                               (const void**)&dp[p].indices_n, (const void**)&dp[p].data_n, (const void**)&dp[p].target_map, (const void**)&dp[p].sample_map};
        if (c.nnz_a >= (1ull << 31) || c.nnz_n >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "combine: part %u exceeds the .bin format's int32 limits", p);
        for (int k = 0; k < 8; ++k)
            if (src[k]) { in.push_back({&bufs[(u64)p * 8 + k], src[k], len[k]}); at.push_back(dst[k]); }
        R += c.n_ecs; NP += c.nnz_a; NZ += c.nnz_n;
    }
    RCCHK(stage_in(c, in));
    for (size_t i = 0; i < in.size(); ++i) *at[i] = in[i].d->p;
    DevBuf<> oia, oxa, oda, oin, oxn, odn;
    const u64 nptr = ((u64)n_samples + 1) * 4;
    int rc = stage_in(c, {{&oia, nullptr, (R + 1) * 4}, {&oxa, nullptr, NP * 4}, {&oda, nullptr, NP * 4}, {&oin, nullptr, nptr}, {&oxn, nullptr, NZ * 4},
                      {&odn, nullptr, NZ * 4}});
    if (rc == ECB_OK) rc = ecb_combine_device(device, n_parts, dp.data(), n_loci, n_haps, n_samples, oia.p, oxa.p, oda.p, oin.p, oxn.p, odn.p, out_sizes);
    RCCHK(rc);
    const u64 E = out_sizes[0], nnz_a = out_sizes[1], nnz_n = out_sizes[2];
    return stage_out(c, {{out_indptr_a, &oia, (E + 1) * 4}, {out_indptr_n, &oin, nptr}, {out_indices_a, &oxa, nnz_a * 4}, {out_data_a, &oda, nnz_a * 4},
                         {out_indices_n, &oxn, nnz_n * 4}, {out_data_n, &odn, nnz_n * 4}});
}

// ---- ecbundle: a .bin's columns collapsed into groups, its rows folded back into ECs (ecb_bundle / ecb_bundle_device) -------------------
// The reference's AlignmentPropertyMatrix.bundle(reset=True) (AlignmentPropertyMatrix.py:219-275: every haplotype's matrix times a T x G
// incidence matrix, the values reset to 1) followed by the merge of the one result.  The group map is many-to-one, one-to-none and
// one-to-many at once, so a non-zero becomes as many (row, group) pairs as its locus has groups, and pairs that land on one (row, group)
// have their masks OR-ed.  In front of cb_finish:
//   k_bd_map_ptr / k_bd_map_idx   the map's pointers, then its group ids (range, ascending within a locus)
//   k_bd_count     one thread per non-zero: checked as k_cb_pairs checks it; its row and the number of groups of its locus
//   scan           the non-zeros' first places among the expanded pairs
//   k_bd_expand    one thread per EXPANDED pair: its non-zero by binary search in the scan, key = row << 32 | group, value = mask
//   radix_sort_pairs64 on the row and group bits;  k_run_heads + scan: the runs of equal (row, group)
//   k_bd_fold      one thread per sorted pair: the OR of a run's masks by a segmented wave scan (the run's first lane from the ballot of
//                  the head flags: six 32-bit shuffles, no key compares), one write per run and wave -- a plain store when the run lies
//                  within the wave, an atomic OR into zeroed storage when it goes on in a neighbouring one
//   k_bd_rowptr    the folded rows' places: a binary search per row
// No kernel loops over a row, a group or a locus's group list: 10 000 members of one gene in a row cost what 10 000 rows of one pair do.
namespace {
constexpr u32 BD_MAX_GROUPS_PER_LOCUS = 65535;       // (a scan stretch of 16 384 counts sums in 32 bits)
constexpr int BD_FOLD_TPB = TPB, BD_WAVE = 64;       // the fold's workgroup, and the wave a run is folded within
__global__ __launch_bounds__(TPB) void k_bd_map_ptr(const u32* mptr, u32 n_loci, u64 n_map, u32* err) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    u32 e = 0;
    if (k <= n_loci) {
        if (cb_ptr_bad(reinterpret_cast<const int*>(mptr), k, n_loci, n_map)) e |= BD_ERR_MPTR;
        else if (k < n_loci && mptr[k + 1] - mptr[k] > BD_MAX_GROUPS_PER_LOCUS) e |= BD_ERR_WIDE;
    }
    cb_raise(e, err);
}
__global__ __launch_bounds__(TPB) void k_bd_map_idx(const u32* mptr, const u32* midx, u32 n_loci, u64 n_map, u32 n_groups, u32* err) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    u32 e = 0;
    if (j < n_map) {
        const u32 g = midx[j];
        if (g >= n_groups) e |= BD_ERR_MIDX;
        const u32 c = cb_row(reinterpret_cast<const int*>(mptr), n_loci, (long long)j);
        if (j > mptr[c] && midx[j - 1] >= g) e |= BD_ERR_MORDER;
    }
    cb_raise(e, err);
}
__global__ __launch_bounds__(TPB) void k_bd_count(const CbPart* P, u32 n_haps, const u32* mptr, u32* cnt, u32* row, u32* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const CbPart& q = P[0];
    u32 e = 0;
    if (i < q.nnz_a) {
        const u32 r = cb_row(q.ipa, q.n_ecs, (long long)i);
        const int c = q.ixa[i];
        e = cb_nz_bad(q, (long long)i, r, n_haps, c, (u32)q.daa[i]);
        cnt[i] = (e & CB_ERR_LOCUS) ? 0u : mptr[c + 1] - mptr[c];
        row[i] = r;
    }
    cb_raise(e, err);
}
// (first[i] = the first expanded pair of non-zero i, first[nnz] = n: the largest i with first[i] <= x is the one that has pair x)
__global__ __launch_bounds__(TPB) void k_bd_expand(const CbPart* P, const u32* first, const u32* row, const u32* mptr, const u32* midx, u64 n,
                                                   u64* keys, u32* vals) {
    const u64 x = blockIdx.x * (u64)TPB + threadIdx.x;
    if (x >= n) return;
    const CbPart& q = P[0];
    u64 a = 0, b = q.nnz_a;
    while (b - a > 1) { const u64 m = (a + b) >> 1; if (first[m] <= x) a = m; else b = m; }
    const u32 g = midx[mptr[q.ixa[a]] + ((u32)x - first[a])];
    keys[x] = ((u64)row[a] << 32) | g;
    vals[x] = (u32)q.daa[a];
}
__global__ __launch_bounds__(BD_FOLD_TPB) void k_bd_fold(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u64* okeys,
                                                         u32* ovals) {
    const u64 i = blockIdx.x * (u64)BD_FOLD_TPB + threadIdx.x;
    const u32 lane = threadIdx.x & (BD_WAVE - 1u);
    const bool valid = i < n;
    u32 f = 1, v = 0, at = 0;                            // (the lanes past the end are runs of their own)
    if (valid) {
        f = flag[i]; v = vals[i];
        at = pos[i] + f - 1u;
        if (f) okeys[at] = keys[i];
    }
    const u64 heads = __ballot(f != 0u) | 1ull;          // where a run starts within this wave
    const u32 f0 = (u32)__builtin_amdgcn_readfirstlane((int)f);
    const u32 s = 63u - (u32)__builtin_clzll(heads & (~0ull >> (63u - lane)));      // the first lane of this lane's run
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const u32 ov = (u32)__shfl_up((int)v, d);
        if (lane >= s + d) v |= ov;
    }
    if (!valid || (lane != 63u && !((heads >> (lane + 1u)) & 1ull))) return;       // not the run's last lane in this wave
    const bool before = s == 0u && f0 == 0u;             // the run began in the wave before
    const bool after = lane == 63u && i + 1 < n && flag[i + 1] == 0u;
    if (before || after) atomicOr(ovals + at, v);
    else ovals[at] = v;
}
__global__ void k_bd_rowptr(const u64* keys, u64 n, u32 n_rows, u32* rowptr) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r <= n_rows) rowptr[r] = (u32)lower_bound_u64(keys, n, r << 32);
}
}  // namespace

extern "C" int ecb_bundle_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint32_t n_groups, uint64_t nnz_a,
                                 const void* d_indptr_a, const void* d_indices_a, const void* d_data_a, uint64_t nnz_n, const void* d_indptr_n,
                                 const void* d_indices_n, const void* d_data_n, uint64_t n_map, const void* d_map_ptr, const void* d_map_idx,
                                 uint64_t a_capacity, void* d_out_indptr_a, void* d_out_indices_a, void* d_out_data_a, void* d_out_indptr_n,
                                 void* d_out_indices_n, void* d_out_data_n, uint64_t* out_sizes) {
    if (!out_sizes || !d_indptr_a || !d_indptr_n || !d_map_ptr || !d_out_indptr_a || !d_out_indptr_n || !n_loci || !n_groups || !n_haps || n_haps > 31 ||
        (nnz_a && (!d_indices_a || !d_data_a)) || (nnz_n && (!d_indices_n || !d_data_n)) || (n_map && !d_map_idx))
        return fail(nullptr, ECB_ERR_ARG, "bundle: bad argument");
    if (n_groups >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "bundle: n_groups out of range (1 .. 2^26-3)");
    if (nnz_a >= (1ull << 31) || nnz_n >= (1ull << 30) || n_map >= (1ull << 31) || n_ecs >= (1u << 31) - 1u || n_loci >= (1u << 31) - 1u ||
        n_samples >= (1u << 31) - 1u)
        return fail(nullptr, ECB_ERR_LIMIT, "bundle: the sizes exceed the .bin format's int32 limits");
    if ((n_ecs && a_capacity && (!d_out_indices_a || !d_out_data_a)) || (nnz_n && (!d_out_indices_n || !d_out_data_n)))
        return fail(nullptr, ECB_ERR_ARG, "bundle: null output");
    const u32 *mptr = (const u32*)d_map_ptr, *midx = (const u32*)d_map_idx;
    const CbPart hp{(const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a, (const int*)d_indptr_n, (const int*)d_indices_n,
                    (const int*)d_data_n, nullptr, nullptr, n_ecs, n_loci, n_samples, 0u, nnz_a, nnz_n};
    u64 base[CB_BASES * 2];                              // one part: every base array is {0, its size}
    const u64 add[CB_BASES] = {n_ecs, nnz_a, nnz_n, (u64)n_ecs + 1, (u64)n_samples + 1};
    for (int k = 0; k < CB_BASES; ++k) { base[2 * k] = 0; base[2 * k + 1] = add[k]; }
    Call c(device, "bundle: ", true); if (c.rc) return c.rc;
    hipStream_t& st = c.st;
    CbRun w{};
    w.n_parts = 1; w.n_loci = n_groups; w.n_haps = n_haps; w.n_samples = n_samples; w.R = n_ecs; w.NZ = nnz_n;
    CbPart* d_parts = c.get<CbPart>(1);
    u64 *d_base = c.get<u64>(CB_BASES * 2), *tot = c.get<u64>(2);
    w.d_parts = d_parts; w.d_base = d_base;
    w.words = c.get<u64>(CB_WORDS);
    u32 *cnt = c.get<u32>(nnz_a), *first = c.get<u32>(nnz_a + 1), *row = c.get<u32>(nnz_a), *sums = c.get<u32>(scan_words(nnz_a));
    RCCHK(c.missing());
    CALLCHK(c, hipMemcpyAsync(d_parts, &hp, sizeof(CbPart), hipMemcpyHostToDevice, st));
    CALLCHK(c, hipMemcpyAsync(d_base, base, sizeof(base), hipMemcpyHostToDevice, st));
    CALLCHK(c, hipMemsetAsync(w.words, 0, CB_WORDS * 8, st));
    CALLCHK(c, hipMemsetAsync(tot, 0, 16, st));
    // 1. the pointers of A, N and the map; then what trusts them: the map's group ids, and 2. the non-zeros
    k_cb_check<<<nblk(std::max<u64>(n_ecs, n_samples) + 1, TPB), TPB, 0, st>>>(d_parts, 1, d_base, w.err());
    k_bd_map_ptr<<<nblk((u64)n_loci + 1, TPB), TPB, 0, st>>>(mptr, n_loci, n_map, w.err());
    RCCHK(cb_refusal(c, w));
    if (n_map) k_bd_map_idx<<<nblk(n_map, TPB), TPB, 0, st>>>(mptr, midx, n_loci, n_map, n_groups, w.err());
    if (nnz_a) k_bd_count<<<nblk(nnz_a, TPB), TPB, 0, st>>>(d_parts, n_haps, mptr, cnt, row, w.err());
    RCCHK(cb_refusal(c, w));
    // 3. the expanded pairs
    u64 X = 0, NC = 0;
    if (nnz_a) {
        CALLCHK(c, scan_launch(st, cnt, nnz_a, first, sums, tot, 1, first + nnz_a));
        CALLCHK(c, hipMemcpyAsync(&X, tot, 8, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
    }
    if (X >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "bundle: 2^30 (row, group) pairs or more before the fold");      // (radix_sort_pairs64)
    const u64 NK = std::max<u64>(X, nnz_n);
    w.keys0 = c.get<u64>(NK); w.keys1 = c.get<u64>(NK); w.vals0 = c.get<u32>(NK); w.vals1 = c.get<u32>(NK);
    u32* rowptr = c.get<u32>((u64)n_ecs + 1);
    w.rowhash = c.get<u64>(n_ecs); w.ent = c.get<Entry>(n_ecs);
    RCCHK(c.missing());
    u64* ckeys = nullptr; u32* cvals = nullptr;
    if (X) {
        u32 *flag = c.get<u32>(X), *pos = c.get<u32>(X + 1), *sums2 = c.get<u32>(scan_words(X));
        SortScratch sc{c.get<u32>(rs_words(X)), c.get<u32>(RS_AUX_WORDS), w.words + 1};
        RCCHK(c.missing());
        k_bd_expand<<<nblk(X, TPB), TPB, 0, st>>>(d_parts, first, row, mptr, midx, X, w.keys0, w.vals0);
        // 4. (row, group) order; 5. the runs of equal (row, group)
        SortBufs s{{w.keys0, w.keys1}, {w.vals0, w.vals1}};
        CALLCHK(c, radix_sort_pairs64(st, s, X, sc, msb_mask((u64)(n_ecs - 1) << 32 | (n_groups - 1))));
        k_run_heads<<<nblk(X, TPB), TPB, 0, st>>>(s.keys(), X, flag);
        CALLCHK(c, scan_launch(st, flag, X, pos, sums2, tot + 1));
        CALLCHK(c, hipMemcpyAsync(&NC, tot + 1, 8, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
        if (NC > X) return fail(nullptr, ECB_ERR_HIP, "internal: %llu runs from %llu pairs", (unsigned long long)NC, (unsigned long long)X);
        if (NC > a_capacity)
            return fail(nullptr, ECB_ERR_ARG, "bundle: %llu non-zeros after the fold, room for %llu", (unsigned long long)NC, (unsigned long long)a_capacity);
        // 6. one mask per run, the compacted pairs
        ckeys = c.get<u64>(NC); cvals = c.get<u32>(NC);
        RCCHK(c.missing());
        CALLCHK(c, hipMemsetAsync(cvals, 0, NC * 4, st));
        k_bd_fold<<<nblk(X, BD_FOLD_TPB), BD_FOLD_TPB, 0, st>>>(s.keys(), s.vals(), flag, pos, X, ckeys, cvals);
    } else {
        ckeys = c.get<u64>(0); cvals = c.get<u32>(0);
    }
    w.pairs = c.get<uint2>(NC);
    RCCHK(c.missing());
    k_bd_rowptr<<<nblk((u64)n_ecs + 1, TPB), TPB, 0, st>>>(ckeys, NC, n_ecs, rowptr);
    CALLCHK(c, hipMemsetAsync(w.rowhash, 0, std::max<u64>(n_ecs, 1) * 8, st));
    CALLCHK(c, hipGetLastError());
    w.NP = NC; w.keys = ckeys; w.vals = cvals; w.rowptr = rowptr;
    return cb_finish(c, w, d_out_indptr_a, d_out_indices_a, d_out_data_a, d_out_indptr_n, d_out_indices_n, d_out_data_n, out_sizes);
}

extern "C" int ecb_bundle(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint32_t n_samples, uint32_t n_groups, uint64_t nnz_a,
                          const int32_t* indptr_a, const int32_t* indices_a, const int32_t* data_a, uint64_t nnz_n, const int32_t* indptr_n,
                          const int32_t* indices_n, const int32_t* data_n, uint64_t n_map, const uint32_t* map_ptr, const uint32_t* map_idx,
                          uint64_t a_capacity, int32_t* out_indptr_a, int32_t* out_indices_a, int32_t* out_data_a, int32_t* out_indptr_n,
                          int32_t* out_indices_n, int32_t* out_data_n, uint64_t* out_sizes) {
    if (!out_sizes || !indptr_a || !indptr_n || !map_ptr || !out_indptr_a || !out_indptr_n) return fail(nullptr, ECB_ERR_ARG, "bundle: bad argument");
    if (nnz_a >= (1ull << 31) || nnz_n >= (1ull << 31) || n_map >= (1ull << 31) || a_capacity >= (1ull << 31))
        return fail(nullptr, ECB_ERR_LIMIT, "bundle: the sizes exceed the .bin format's int32 limits");
    Call c(device, "bundle: "); if (c.rc) return c.rc;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, mp, mi, oia, oxa, oda, oin, oxn, odn;
    const u64 nptr = ((u64)n_samples + 1) * 4;
    int rc = stage_in(c, {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz_a * 4}, {&daa, data_a, nnz_a * 4}, {&ipn, indptr_n, nptr},
                          {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4}, {&mp, map_ptr, ((u64)n_loci + 1) * 4}, {&mi, map_idx, n_map * 4},
                          {&oia, nullptr, ((u64)n_ecs + 1) * 4}, {&oxa, nullptr, a_capacity * 4}, {&oda, nullptr, a_capacity * 4}, {&oin, nullptr, nptr},
                          {&oxn, nullptr, nnz_n * 4}, {&odn, nullptr, nnz_n * 4}});
    if (rc == ECB_OK) rc = ecb_bundle_device(device, n_ecs, n_loci, n_haps, n_samples, n_groups, nnz_a, ipa.p, ixa.p, daa.p, nnz_n, ipn.p, ixn.p, dan.p,
                                             n_map, mp.p, mi.p, a_capacity, oia.p, oxa.p, oda.p, oin.p, oxn.p, odn.p, out_sizes);
    RCCHK(rc);
    const u64 E = out_sizes[0], na = out_sizes[1], nn = out_sizes[2];
    return stage_out(c, {{out_indptr_a, &oia, (E + 1) * 4}, {out_indptr_n, &oin, nptr}, {out_indices_a, &oxa, na * 4}, {out_data_a, &oda, na * 4},
                         {out_indices_n, &oxn, nn * 4}, {out_data_n, &odn, nn * 4}});
}

// ---- salmon2ec: CSR A and N of a salmon eq_classes.txt EC section (ecb_salmon_ecs / ecb_salmon_ecs_device) ------------------------------
// (salmon_utils.py:31-127: every EC line `k t_1 .. t_k count`, each target id -> (transcript, haplotype); A[row, transcript] = sum of 2^h over
//  the line's targets, columns ascending; N = the non-zero counts.)  No serial walk over lines and no per-byte atomics:
//   k_sl_count   one workgroup per 4 KB tile (16 bytes per thread, one 16-byte load): its line ends and field starts (a digit after a
//                non-digit), one pair of counts per tile; the library's one-pass scan (scan_launch) turns them into each tile's first line
//                and first field
//   k_sl_place   the tile again: every byte checked with its neighbours, every line end writes its line's field end, and every field is
//                parsed by the thread that holds its first digit (into the next thread's bytes when it runs on) -> value and line per field
//   k_sl_fields  one thread per field: the line's field range says what it is (k, target id or count); k and the targets are checked,
//                a target becomes (row << 32 | column << 5 | haplotype, 1 << haplotype), a count goes to its line
//   radix_sort_pairs64 on the row and column bits only (rows come in order, the sort orders the columns within them); the haplotype
//   rides in the key's low 5 bits, so a target id repeated in a line is an equal neighbour after the sort
//   k_sl_heads   head flags of the (row, column) runs, repeats refused; scan; k_sl_emit ORs each run's bits (a run holds at most n_haps
//                pairs) into one non-zero; k_sl_rowptr row pointers by binary search; k_sl_nkeep / scan / k_sl_nemit: N
// A refusal names the lowest offending line: every check does an atomicMin of (line << 8 | reason) on one word, which only an error
// touches.  The targets of a well-formed text are slot f - 2 l - 1 of field f in line l (k and the count of every line before it are not
// targets); when some line is malformed that numbering does not hold, and the fields go once more into one slot each (the non-targets as
// a key that sorts last) so that repeats are still found in the lines before the first malformed one.
namespace {
using u8 = unsigned char;
constexpr u32 SL_TILE = TPB * 16;                         // bytes per workgroup of k_sl_count / k_sl_place
constexpr u32 SL_NONE = 256u;                             // "no byte" (before the start, after the end): not a digit, not a separator
enum : u32 { SL_R_BYTE = 1, SL_R_EMPTY, SL_R_BIG, SL_R_FEW, SL_R_K, SL_R_TARGET, SL_R_REPEAT, SL_R_COUNT };
const char* sl_reason(u32 r) {
    switch (r) {
    case SL_R_BYTE: return "a byte other than a digit, tab or line end";
    case SL_R_EMPTY: return "an empty field";
    case SL_R_BIG: return "a value of 2^31 or more";
    case SL_R_FEW: return "fewer than 2 fields";
    case SL_R_K: return "k differs from the number of target ids";
    case SL_R_TARGET: return "a target id at or beyond the number of targets";
    case SL_R_REPEAT: return "a target id repeated within the line";
    case SL_R_COUNT: return "the number of EC lines differs from the header's";
    default: return "unknown";
    }
}
__device__ __forceinline__ bool sl_digit(u32 c) { return c - 48u < 10u; }
// value * 10 + digit, held at 2^31 once it gets there (every value from 2^31 on is refused alike)
__device__ __forceinline__ u32 sl_acc(u32 acc, u32 c) { const u64 x = (u64)acc * 10u + (c - 48u); return x < (1ull << 31) ? (u32)x : 1u << 31; }
// the 16 bytes at base (zero past the end), and the bytes just before and after them (SL_NONE outside the text)
__device__ __forceinline__ void sl_load(const u8* text, u64 L, u64 base, u32 w[4], u32& prev, u32& next) {
    if (base + 16 <= L && (reinterpret_cast<uintptr_t>(text + base) & 15u) == 0u) {
        const uint4 q = *reinterpret_cast<const uint4*>(text + base);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (base + k < L) w[k >> 2] |= (u32)text[base + k] << (8 * (k & 3));
    }
    prev = base > 0 && base - 1 < L ? (u32)text[base - 1] : SL_NONE;
    next = base + 16 < L ? (u32)text[base + 16] : SL_NONE;
}
__device__ __forceinline__ u32 sl_byte(const u32 w[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }
// line ends and field starts among this thread's 16 bytes
__device__ __forceinline__ void sl_counts(const u32 w[4], u32 prev, u64 base, u64 L, u32& nl, u32& fs) {
    nl = 0; fs = 0;
    u32 pc = prev;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u32 c = base + j < L ? sl_byte(w, j) : SL_NONE;
        nl += c == 10u;
        fs += sl_digit(c) && !sl_digit(pc);
        pc = c;
    }
}
// exclusive prefix of a and b over the workgroup's threads, and the workgroup's totals
__device__ __forceinline__ void sl_block_scan(u32& a, u32& b, u32& ta, u32& tb) {
    __shared__ u32 s_a[TPB / 64], s_b[TPB / 64];
    const u32 ia = wave_incl_scan(a), ib = wave_incl_scan(b), w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) { s_a[w] = ia; s_b[w] = ib; }
    __syncthreads();
    u32 pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (u32 k = 0; k < TPB / 64; ++k) { if (k < w) { pa += s_a[k]; pb += s_b[k]; } ta += s_a[k]; tb += s_b[k]; }
    a = pa + ia - a; b = pb + ib - b;
}
__global__ __launch_bounds__(TPB) void k_sl_count(const u8* text, u64 L, u32* blk_nl, u32* blk_fs) {
    const u64 base = blockIdx.x * (u64)SL_TILE + threadIdx.x * 16ull;
    u32 w[4], prev, next, nl = 0, fs = 0;
    if (base < L) {
        sl_load(text, L, base, w, prev, next);
        sl_counts(w, prev, base, L, nl, fs);
    }
    u32 ta, tb;
    sl_block_scan(nl, fs, ta, tb);
    if (threadIdx.x == 0) { blk_nl[blockIdx.x] = ta; blk_fs[blockIdx.x] = tb; }
}
// every byte checked; line l's end writes fend[l] (its fields are [fend[l - 1], fend[l])); field f's value (2^31 for 2^31 and above) and line
__global__ __launch_bounds__(TPB) void k_sl_place(const u8* text, u64 L, const u32* blk_nl, const u32* blk_fs, u32 fs_total, u32* fval, u32* fline,
                                                  u32* fend, u64* err) {
    const u64 base = blockIdx.x * (u64)SL_TILE + threadIdx.x * 16ull;
    u32 w[4] = {0u, 0u, 0u, 0u}, prev = SL_NONE, next = SL_NONE, nl = 0, fs = 0;
    if (base < L) {
        sl_load(text, L, base, w, prev, next);
        sl_counts(w, prev, base, L, nl, fs);
    }
    u32 ta, tb;
    sl_block_scan(nl, fs, ta, tb);
    if (base >= L) return;
    u32 l = blk_nl[blockIdx.x] + nl, f = blk_fs[blockIdx.x] + fs;
    u32 acc = 0;
    bool open = false;                                    // a field whose first digit is ours is being read
    u32 pc = prev;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u64 p = base + j;
        if (p < L) {
            const u32 c = sl_byte(w, j), nc = j < 15 ? (p + 1 < L ? sl_byte(w, j + 1) : SL_NONE) : next;
            if (sl_digit(c)) {
                if (!sl_digit(pc)) { open = true; acc = c - 48u; }
                else if (open) acc = sl_acc(acc, c);
                if (open && !sl_digit(nc)) {
                    fval[f] = acc; fline[f] = l; ++f; open = false;
                }
            } else if (c == 10u) {
                if (!sl_digit(pc) && pc != 13u) offender(err, l, SL_R_EMPTY);
                fend[l] = f; ++l;
            } else if (c == 9u) {
                if (!sl_digit(pc) || !sl_digit(nc)) offender(err, l, SL_R_EMPTY);
            } else if (c == 13u) {
                if (nc != 10u) offender(err, l, SL_R_BYTE);
                else if (!sl_digit(pc)) offender(err, l, SL_R_EMPTY);
            } else {
                offender(err, l, SL_R_BYTE);
            }
            if (p + 1 == L && c != 10u) fend[l] = fs_total;    // (the last line has no line end)
            pc = c;
        }
    }
    if (open) {                                           // our last field runs on into the next thread's bytes
        u64 p = base + 16;
        for (; p < L; ++p) {
            const u32 c = text[p];
            if (!sl_digit(c)) break;
            acc = sl_acc(acc, c);
        }
        fval[f] = acc; fline[f] = l;
    }
}
// field f of line l: k (the first), a target id (between), or the count (the last).  dense: target slot f - 2 l - 1 (exact when every line has
// at least 2 fields; slots out of range are skipped); otherwise slot f for every field, the non-targets (and targets out of range) as ~0.
__global__ __launch_bounds__(TPB) void k_sl_fields(const u32* fval, const u32* fline, const u32* fend, u32 n_fields, u32 n_targets, const u32* tcol,
                                                   const u32* thap, bool dense, u64 n_slots, u64* keys, u32* vals, u32* cnt, u64* err) {
    const u64 f = blockIdx.x * (u64)TPB + threadIdx.x;
    if (f >= n_fields) return;
    const u32 v = fval[f], l = fline[f];
    const u32 f0 = l ? fend[l - 1] : 0u, nf = fend[l] - f0, i = (u32)f - f0;
    if (v >= (1u << 31)) offender(err, l, SL_R_BIG);
    if (i == 0 && nf < 2) offender(err, l, SL_R_FEW);
    else if (i == 0 && v != nf - 2) offender(err, l, SL_R_K);
    if (nf >= 2 && i == nf - 1) cnt[l] = v;
    const bool target = nf >= 2 && i >= 1 && i + 1 < nf;
    u64 key = ~0ull;
    u32 val = 0;
    if (target) {
        if (v >= n_targets) offender(err, l, SL_R_TARGET);
        else { const u32 h = thap[v]; key = (u64)l << 32 | (tcol[v] << 5 | h); val = 1u << h; }
    }
    if (dense) {
        const long long s = (long long)f - 2ll * l - 1;
        if (!target || s < 0 || (u64)s >= n_slots) return;
        keys[s] = key; vals[s] = val;
    } else {
        keys[f] = key; vals[f] = val;
    }
}
__global__ void k_sl_targets(const u32* tcol, const u32* thap, u32 T, u32 n_loci, u32 n_haps, u32* bad) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const bool b = t < T && (tcol[t] >= n_loci || thap[t] >= n_haps);
    if (__ballot(b) && (threadIdx.x & 63u) == 0u) atomicOr(bad, 1u);
}
// sorted keys: flag = first of its (row, column) run; an equal neighbour is a repeated target id
__global__ __launch_bounds__(TPB) void k_sl_heads(const u64* keys, u64 n, u32* flag, u64* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    u32 h = 0;
    if (k != ~0ull) {
        const u64 q = i ? keys[i - 1] : ~0ull;
        if (q == k) offender(err, k >> 32, SL_R_REPEAT);
        h = i == 0 || (q >> 5) != (k >> 5);
    }
    flag[i] = h;
}
__global__ __launch_bounds__(TPB) void k_sl_emit(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u64 cap, int* indices, int* data) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n || !flag[i] || pos[i] >= cap) return;
    const u64 run = keys[i] >> 5;
    u32 m = 0;
    for (u64 j = i; j < n && (keys[j] >> 5) == run; ++j) m |= vals[j];
    indices[pos[i]] = (int)((u32)run & 0x7FFFFFFu);
    data[pos[i]] = (int)m;
}
__global__ void k_sl_rowptr(const u64* keys, u64 n, const u32* pos, u32 n_rows, int* indptr) {
    const u64 r = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (r <= n_rows) indptr[r] = (int)pos[lower_bound_u64(keys, n, r << 32)];
}
__global__ void k_sl_nkeep(const u32* cnt, u32 n, u32* keep) {
    const u64 l = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (l < n) keep[l] = cnt[l] != 0u;
}
__global__ void k_sl_nemit(const u32* cnt, const u32* keep, const u32* pos, u32 n, int* indices, int* data) {
    const u64 l = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (l >= n || !keep[l]) return;
    indices[pos[l]] = (int)l;
    data[pos[l]] = (int)cnt[l];
}
}  // namespace

extern "C" int ecb_salmon_ecs_device(int device, const void* d_text, uint64_t n_bytes, uint32_t n_ecs, uint32_t n_targets, const void* d_target_col,
                                     const void* d_target_hap, uint32_t n_loci, uint32_t n_haps, uint64_t capacity, void* d_out_indptr,
                                     void* d_out_indices, void* d_out_data, void* d_out_n_indices, void* d_out_n_data, uint64_t* out_sizes) {
    if (!out_sizes || !d_out_indptr || (n_bytes && !d_text) || (n_targets && (!d_target_col || !d_target_hap)) || !n_loci || !n_haps || n_haps > 31 ||
        (capacity && (!d_out_indices || !d_out_data)) || (n_ecs && (!d_out_n_indices || !d_out_n_data)))
        return fail(nullptr, ECB_ERR_ARG, "salmon: bad argument");
    if (n_loci >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "salmon: n_loci out of range (1 .. 2^26-3)");
    if (n_ecs >= (1u << 31) - 1u || n_targets >= (1u << 31)) return fail(nullptr, ECB_ERR_LIMIT, "salmon: E or T beyond int32");
    Call c(device, "salmon: ", true); if (c.rc) return c.rc;
    auto refuse = [](u64 e) { const u32 r = (u32)(e & 255u); return fail(nullptr, ECB_ERR_CONTRACT, "EC line %llu: %s (reason %u)", (unsigned long long)(e >> 8), sl_reason(r), r); };
    hipStream_t st = c.st;
    const u8* text = (const u8*)d_text;
    const u32 *tcol = (const u32*)d_target_col, *thap = (const u32*)d_target_hap;
    const u64 L = n_bytes, nb = std::max<u64>(1, (L + SL_TILE - 1) / SL_TILE);
    if (nb >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "salmon: text too long");
    u32 *blk_nl = c.get<u32>(nb), *blk_fs = c.get<u32>(nb), *nl_ex = c.get<u32>(nb), *fs_ex = c.get<u32>(nb);
    u32 *sc1 = c.get<u32>(scan_words(nb)), *sc2 = c.get<u32>(scan_words(nb));
    u64* words;                                        // [0] lowest (line << 8 | reason), [1] [2] line ends, field starts, [3] bad target map, [4] [5] scan totals
    RCCHK(c.status_words(words, 8, 1, true));
    u64* err = words;
    u32* bad = reinterpret_cast<u32*>(words + 3);
    u64 back[8] = {0};
    u8 last = 10;
    // 1. the target map; line ends and field starts per tile, placed
    if (n_targets) k_sl_targets<<<nblk(n_targets, TPB), TPB, 0, st>>>(tcol, thap, n_targets, n_loci, n_haps, bad);
    if (L) {
        k_sl_count<<<(unsigned)nb, TPB, 0, st>>>(text, L, blk_nl, blk_fs);
        CALLCHK(c, scan_launch(st, blk_nl, nb, nl_ex, sc1, words + 1));
        CALLCHK(c, scan_launch(st, blk_fs, nb, fs_ex, sc2, words + 2));
        CALLCHK(c, hipMemcpyAsync(&last, text + L - 1, 1, hipMemcpyDeviceToHost, st));
    }
    RCCHK(c.read_back(back, words, 8));
    if (back[3]) return fail(nullptr, ECB_ERR_CONTRACT, "salmon: the target map has a column at or beyond n_loci or a haplotype at or beyond n_haps");
    const u64 n_lines = back[1] + (L && last != 10), NF = back[2];
    if (NF >= (1ull << 30) || n_lines >= (1ull << 31) - 1) return fail(nullptr, ECB_ERR_LIMIT, "salmon: %llu fields in %llu lines: beyond the limits (2^30, 2^31-1)",
                                                                       (unsigned long long)NF, (unsigned long long)n_lines);
    const u64 count_err = n_lines != n_ecs ? (std::min<u64>(n_lines, n_ecs) << 8 | SL_R_COUNT) : NO_OFFENDER;
    // 2. bytes checked, fields parsed; 3. fields classified, targets to keys (dense slots)
    u32 *fval = c.get<u32>(NF), *fline = c.get<u32>(NF), *fend = c.get<u32>(n_lines), *cnt = c.get<u32>(n_lines);
    u64 *keys0 = c.get<u64>(NF), *keys1 = c.get<u64>(NF);
    u32 *vals0 = c.get<u32>(NF), *vals1 = c.get<u32>(NF), *flag = c.get<u32>(NF), *pos = c.get<u32>(NF + 1), *sc3 = c.get<u32>(scan_words(NF));
    SortScratch ss{c.get<u32>(rs_words(NF)), c.get<u32>(RS_AUX_WORDS), words + 6};
    RCCHK(c.missing());
    if (L) k_sl_place<<<(unsigned)nb, TPB, 0, st>>>(text, L, nl_ex, fs_ex, (u32)NF, fval, fline, fend, err);
    const u64 NP = NF >= 2 * n_lines ? NF - 2 * n_lines : 0;
    if (NF) k_sl_fields<<<nblk(NF, TPB), TPB, 0, st>>>(fval, fline, fend, (u32)NF, n_targets, tcol, thap, true, NP, keys0, vals0, cnt, err);
    RCCHK(c.read_back(back, words, 8));
    SortBufs s{{keys0, keys1}, {vals0, vals1}};
    if (back[0] != NO_OFFENDER) {
        // a malformed line: every field in a slot of its own, sorted on all bits, so that repeats in the lines before it are found too
        k_sl_fields<<<nblk(NF, TPB), TPB, 0, st>>>(fval, fline, fend, (u32)NF, n_targets, tcol, thap, false, NF, keys0, vals0, cnt, err);
        CALLCHK(c, radix_sort_pairs64(st, s, NF, ss));
        k_sl_heads<<<nblk(NF, TPB), TPB, 0, st>>>(s.keys(), NF, flag, err);
        RCCHK(c.read_back(back, words, 8));
        return refuse(std::min(back[0], count_err));
    }
    // 4. sort within rows (the row and column bits only); runs, repeats refused
    const u64 mask = msb_mask(n_lines ? n_lines - 1 : 0) << 32 | msb_mask((u64)(n_loci - 1) << 5 | 31u);
    CALLCHK(c, radix_sort_pairs64(st, s, NP, ss, mask));
    const u64* keys = s.keys(); const u32* vals = s.vals();
    if (NP) k_sl_heads<<<nblk(NP, TPB), TPB, 0, st>>>(keys, NP, flag, err);
    CALLCHK(c, scan_launch(st, flag, NP, pos, sc3, words + 4, 1, pos + NP));
    RCCHK(c.read_back(back, words, 8));
    if (std::min(back[0], count_err) != NO_OFFENDER) return refuse(std::min(back[0], count_err));
    const u64 nnz = NP ? back[4] : 0;
    if (nnz > capacity) return fail(nullptr, ECB_ERR_LIMIT, "salmon: %llu non-zeros, room for %llu", (unsigned long long)nnz, (unsigned long long)capacity);
    if (nnz >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "salmon: non-zeros beyond int32");
    // 5. A: one non-zero per run, row pointers; N: the non-zero counts
    if (NP) k_sl_emit<<<nblk(NP, TPB), TPB, 0, st>>>(keys, vals, flag, pos, NP, capacity, (int*)d_out_indices, (int*)d_out_data);
    k_sl_rowptr<<<nblk((u64)n_ecs + 1, TPB), TPB, 0, st>>>(keys, NP, pos, n_ecs, (int*)d_out_indptr);
    if (n_ecs) {
        k_sl_nkeep<<<nblk(n_ecs, TPB), TPB, 0, st>>>(cnt, n_ecs, flag);
        CALLCHK(c, scan_launch(st, flag, n_ecs, pos, sc3, words + 5));
        k_sl_nemit<<<nblk(n_ecs, TPB), TPB, 0, st>>>(cnt, flag, pos, n_ecs, (int*)d_out_n_indices, (int*)d_out_n_data);
    }
    RCCHK(c.read_back(back, words, 8));
    out_sizes[0] = nnz;
    out_sizes[1] = n_ecs ? back[5] : 0;
    return ECB_OK;
}

extern "C" int ecb_salmon_ecs(int device, const char* text, uint64_t n_bytes, uint32_t n_ecs, uint32_t n_targets, const uint32_t* target_col,
                              const uint32_t* target_hap, uint32_t n_loci, uint32_t n_haps, uint64_t capacity, int32_t* out_indptr, int32_t* out_indices,
                              int32_t* out_data, int32_t* out_n_indices, int32_t* out_n_data, uint64_t* out_sizes) {
    if (!out_sizes || !out_indptr || (n_bytes && !text) || (n_targets && (!target_col || !target_hap)) || (capacity && (!out_indices || !out_data)) ||
        (n_ecs && (!out_n_indices || !out_n_data)))
        return fail(nullptr, ECB_ERR_ARG, "salmon: bad argument");
    if (n_ecs >= (1u << 31) - 1u || capacity >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "salmon: E or the capacity beyond int32");
    Call c(device, "salmon: "); if (c.rc) return c.rc;
    DevBuf<> dt, dc, dh, oip, oix, oda, onx, ond;
    const u64 rowb = ((u64)n_ecs + 1) * 4;
    int rc = stage_in(c, {{&dt, text, n_bytes}, {&dc, target_col, (u64)n_targets * 4}, {&dh, target_hap, (u64)n_targets * 4}, {&oip, nullptr, rowb},
                          {&oix, nullptr, capacity * 4}, {&oda, nullptr, capacity * 4}, {&onx, nullptr, (u64)n_ecs * 4}, {&ond, nullptr, (u64)n_ecs * 4}});
    if (rc == ECB_OK) rc = ecb_salmon_ecs_device(device, dt.p, n_bytes, n_ecs, n_targets, dc.p, dh.p, n_loci, n_haps, capacity, oip.p, oix.p, oda.p, onx.p, ond.p, out_sizes);
    RCCHK(rc);
    return stage_out(c, {{out_indptr, &oip, rowb}, {out_indices, &oix, out_sizes[0] * 4}, {out_data, &oda, out_sizes[0] * 4}, {out_n_indices, &onx, out_sizes[1] * 4},
                         {out_n_data, &ond, out_sizes[1] * 4}});
}

// a multisample .bin's rows and cell counts from the records of a kallisto BUS file, on salmon2ec's per-row sort-and-fold kernels
// (ecb_bus_molecules / ecb_bus_molecules_device)
#include "bus.inc"
// ... and those records' barcodes snapped onto a whitelist first (ecb_bus_correct / ecb_bus_correct_device)
#include "bus_correct.inc"
// ... and, for the record streams of bam2ec, a read's best-scoring alignments kept (ecb_best_strata / ecb_best_strata_device)
#include "strata.inc"
// ... and the reads of one molecule made one read (ecb_collapse_umis / ecb_collapse_umis_device)
#include "umi.inc"
// ... and, for a .bin's N, n of a sample's reads kept, drawn without replacement (ecb_downsample / ecb_downsample_device)
#include "ds_key.h"
#include "downsample.inc"

// ---- ecb_merge: the multi-GPU merge for ONE process that drives several GPUs ----------------------------------------------
// shards[r] holds the reads of contiguous read shard r on its own device; `root` is an empty handle (any device).  The same protocol as
// alntools_amd/dist.py runs over RCCL with one process per GPU, here with peer copies (hipMemcpyPeerAsync: xGMI between the GPUs of a
// node) -- cut every shard's table into n key ranges, range q of every shard to device q, merged there in shard order on a handle of its own,
// finalized there (ranked against the whole run's read numbering, rows emitted), the finished pieces placed by first read on the root.
// (bam_utils.py:646-724: contiguous chunks per worker, the workers' dicts merged in order.)  Everything is built from the entry points above;
// the devices work one after the other here -- a host that wants them side by side runs one thread or one process per GPU over the same calls.
namespace {
#define MERGECHK(call) HIPCHK_AS(root, "ecb_merge: ", call)
// max(bytes, 16) bytes on device `device` (left current)
int take(ecb_handle* root, DevBuf<>& b, int device, u64 bytes) { MERGECHK(hipSetDevice(device)); MERGECHK(b.alloc(bytes, 16)); return ECB_OK; }
// one key range's finished result: row pointers, columns, masks, counts and first reads, each in a buffer of its own
struct Piece {
    DevBuf<> buf[5]; u64 n_ecs = 0, nnz = 0;
    u64 bytes(int k) const { return k == 0 ? (n_ecs + 1) * 4 : (k <= 2 ? nnz : n_ecs) * 4; }
};
}  // namespace

extern "C" int ecb_merge(ecb_handle* const* shards, uint32_t n, ecb_handle* root, ecb_sizes* out) {
    if (!shards || !n || !root || !out) return fail(root, ECB_ERR_ARG, "ecb_merge: null argument");
    if (n > MAX_PARTS) return fail(root, ECB_ERR_LIMIT, "ecb_merge: at most %u shards", MAX_PARTS);
    RCCHK(refused_run(root));
    for (u32 r = 0; r < n; ++r) {
        if (!shards[r] || shards[r] == root) return fail(root, ECB_ERR_ARG, "ecb_merge: shard %u is null or the root itself", r);
        if (const int rc = refused_run(shards[r])) return fail(root, rc, "ecb_merge: shard %u: %s", r, ecb_last_error(shards[r]));
        if (shards[r]->cfg.n_loci != root->cfg.n_loci || shards[r]->cfg.n_haplotypes != root->cfg.n_haplotypes)
            return fail(root, ECB_ERR_ARG, "ecb_merge: shard %u was created for other targets than the root", r);
        if ((shards[r]->cfg.flags | root->cfg.flags) & ECB_F_MULTISAMPLE) return fail(root, ECB_ERR_STATE, "ecb_merge: single-sample handles (the multisample merge has a second exchange: alntools_amd/dist.py)");
    }
    // 1. every shard: sizes, counters, its table cut into n key ranges (first reads counted from the shard's own 0)
    std::vector<u64> ne(n), np(n), nr(n), all(n), valid(n), base(n + 1, 0);
    std::vector<DevBuf<>> ent(n), prs(n);
    std::vector<std::vector<uint64_t>> eoff(n, std::vector<uint64_t>(n + 1, 0)), poff(n, std::vector<uint64_t>(n + 1, 0));
    for (u32 r = 0; r < n; ++r) {
        uint64_t a = 0, b = 0, c = 0, ca = 0, cv = 0, cr = 0;
        int rc = ecb_table_sizes(shards[r], &a, &b, &c);
        if (rc == ECB_OK) rc = ecb_counters(shards[r], &ca, &cv, &cr);
        if (rc != ECB_OK) return fail(root, rc, "ecb_merge: shard %u: %s", r, ecb_last_error(shards[r]));
        ne[r] = a; np[r] = b; nr[r] = c; all[r] = ca; valid[r] = cv;
        base[r + 1] = base[r] + nr[r];
        RCCHK(take(root, ent[r], shards[r]->device, std::max<u64>(ne[r], 1) * sizeof(Entry)));
        RCCHK(take(root, prs[r], shards[r]->device, std::max<u64>(np[r], 1) * sizeof(uint2)));
        if (ne[r]) {
            rc = ecb_table_export_parts_device(shards[r], ent[r].p, prs[r].p, 0, n, eoff[r].data(), poff[r].data());
            if (rc != ECB_OK) return fail(root, rc, "ecb_merge: shard %u: %s", r, ecb_last_error(shards[r]));
        }
    }
    u64 t_all = 0, t_valid = 0;
    for (u32 r = 0; r < n; ++r) { t_all += all[r]; t_valid += valid[r]; }
    const u64 t_reads = base[n];
    // 2. range q: its pieces to device q (the device of shard q), merged in shard order on a handle of its own, finalized there
    HandleGuard parts;
    std::vector<Piece> piece(n);
    for (u32 q = 0; q < n; ++q) {
        const int dq = shards[q]->device;
        ecb_config cfg = shards[q]->cfg;
        cfg.flags = 0; cfg.device = dq;
        u64 arriving = 0;
        for (u32 r = 0; r < n; ++r) arriving += eoff[r][q + 1] - eoff[r][q];
        if (!arriving) continue;
        cfg.ec_capacity = std::max<u64>(next_pow2(arriving * 2 + 1024), 1 << 12);
        ecb_handle* part = nullptr;
        int rc = ecb_create(&cfg, &part);
        if (rc != ECB_OK) return fail(root, rc, "ecb_merge: range %u: %s", q, ecb_last_error(nullptr));
        parts.h.push_back(part);
        std::vector<DevBuf<>> pe(n), pp(n);
        std::vector<const void*> le, lp; std::vector<uint64_t> lne, lnp;
        for (u32 r = 0; r < n; ++r) {
            const u64 e_n = eoff[r][q + 1] - eoff[r][q], p_n = poff[r][q + 1] - poff[r][q];
            if (!e_n) continue;
            RCCHK(take(root, pe[r], dq, e_n * sizeof(Entry)));
            RCCHK(take(root, pp[r], dq, std::max<u64>(p_n, 1) * sizeof(uint2)));
            MERGECHK(hipMemcpyPeer(pe[r].p, dq, (const char*)ent[r].p + eoff[r][q] * sizeof(Entry), shards[r]->device, e_n * sizeof(Entry)));
            if (p_n) MERGECHK(hipMemcpyPeer(pp[r].p, dq, (const char*)prs[r].p + poff[r][q] * sizeof(uint2), shards[r]->device, p_n * sizeof(uint2)));
            if (base[r]) { rc = ecb_table_rebase_device(part, pe[r].p, e_n, base[r]); if (rc != ECB_OK) return fail(root, rc, "ecb_merge: %s", ecb_last_error(part)); }
            le.push_back(pe[r].p); lp.push_back(pp[r].p); lne.push_back(e_n); lnp.push_back(p_n);
        }
        rc = ecb_table_merge_batch_device(part, (uint32_t)le.size(), le.data(), lne.data(), lp.data(), lnp.data());
        if (rc == ECB_OK) rc = ecb_add_counters(part, t_all, t_valid, t_reads);
        ecb_sizes s{};
        if (rc == ECB_OK) rc = ecb_finalize(part, &s);
        if (rc != ECB_OK) return fail(root, rc, "ecb_merge: range %u: %s", q, ecb_last_error(part));
        Piece& P = piece[q];
        P.n_ecs = s.n_ecs; P.nnz = s.nnz_a;
        for (int k = 0; k < 5; ++k) RCCHK(take(root, P.buf[k], dq, P.bytes(k)));
        rc = ecb_export_device(part, P.buf[0].p, P.buf[1].p, P.buf[2].p, nullptr, nullptr, P.buf[3].p);
        if (rc == ECB_OK) rc = ecb_export_firsts_device(part, P.buf[4].p);
        if (rc != ECB_OK) return fail(root, rc, "ecb_merge: range %u: %s", q, ecb_last_error(part));
    }
    // 3. the finished pieces to the root's device, placed by first read
    const int d0 = root->device;
    std::vector<Piece> at_root(n);
    std::vector<const void*> lst[5]; std::vector<uint64_t> lne2, lnz;
    for (u32 q = 0; q < n; ++q) {
        Piece& S = piece[q];
        if (!S.n_ecs) continue;
        Piece* use = &S;
        if (S.buf[0].dev != d0) {
            Piece& D = at_root[q];
            D.n_ecs = S.n_ecs; D.nnz = S.nnz;
            for (int k = 0; k < 5; ++k) {
                if (const int rc = take(root, D.buf[k], d0, D.bytes(k))) return rc;
                MERGECHK(hipMemcpyPeer(D.buf[k].p, d0, S.buf[k].p, S.buf[0].dev, S.bytes(k)));
            }
            use = &D;
        }
        for (int k = 0; k < 5; ++k) lst[k].push_back(use->buf[k].p);
        lne2.push_back(use->n_ecs); lnz.push_back(use->nnz);
    }
    return ecb_assemble_ranges_device(root, (uint32_t)lst[0].size(), lst[0].data(), lst[1].data(), lst[2].data(), lst[3].data(), lst[4].data(), lne2.data(), lnz.data(),
                                      t_reads, t_all, t_valid, out);
}
