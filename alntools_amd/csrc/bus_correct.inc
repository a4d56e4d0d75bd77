// ---- bus2ec -w / buscorrect: the barcodes of a BUS file's records snapped onto a whitelist (ecb_bus_correct / ecb_bus_correct_device;
// included by ecb.hip after bus.inc, whose record layout and record reasons it shares) ------------------------------------------------------
// bustools correct's rule (include/ecb_bus_correct.h).  Every step is a map over an array or one of the library's scans (scan_launch);
// nothing is placed by an atomic, so every output is a function of the input alone.  The only atomics are the atomicMin of the lowest
// offender (offender, ecb.hip), which only a refusal reads.
//   The lookup.  A real whitelist -- 6.8 M entries, 54 MB -- lives in the Infinity Cache, where a dependent load is some 545 cycles: a
//      bisection of the whole list is 23 of them in a row.  Instead a DIRECTORY over the barcode's leading bits holds one offset per
//      prefix: dir[p] = the first entry whose leading `bits` bits are at or above p, dir[2^bits] = n_white (k_busc_dir: a bisection per
//      directory entry, once per call).  A lookup (busc_has) is one directory read -- dir[p] and dir[p + 1], neighbours -- and the
//      bucket's entries, whose addresses are known together: a bucket of up to BUSC_BISECT_LEN entries is read whole, without an early
//      exit, so its loads are in flight at once; a longer one -- a whitelist whose entries share a prefix -- is bisected.
//      The directory's bit count (busc_dir_bits):
//          bits = the smallest b with n_white <= BUSC_BUCKET_AVG << b, at most min(2 x bclen, BUSC_DIR_MAX_BITS)
//      so an average bucket holds between BUSC_BUCKET_AVG / 2 and BUSC_BUCKET_AVG entries (6.8 M entries: 21 bits, 8 MB of offsets), a
//      whitelist of up to BUSC_BUCKET_AVG entries has no directory bits at all (one bucket), and the directory stays at or below 64 MB.
//      prefix(bc) = bc >> (2 x bclen - bits); bits = 0: prefix 0, and no shift by 64 is ever taken.
//   0. k_busc_white: the whitelist checked, the lowest offending entry by an atomicMin of (index << 8 | reason).  || read back: refusal.
//      k_busc_dir.
//   1. k_busc_exact: a map over the records: the barcode checked (the lowest offender as in k_bus_check; a barcode that fails is not
//      looked up: its prefix would lie beyond the directory), the exact lookup -> status ECB_BUS_EXACT or "miss"; the misses flagged, the
//      library's scan lists them (k_busc_list).  || read back: refusal, the number of misses.
//   2. k_busc_neigh, the hot path: ONE WAVE PER MISS (BUSC_LANES = 64).  Lane l of round r holds neighbour q = 64 r + l < 3 x bclen: base
//      q / 3 (counted from the last base) XOR 1 + q % 3 -- either bit differs --, and looks it up, so a record's lookups are in flight
//      together, not one behind the other in a lane.  A 64-bit __ballot gives the hits; bclen 22 .. 32 takes two rounds.  The hits summed
//      over the rounds: 1 -> ECB_BUS_CORRECTED, and the hit lane stores its neighbour; 0 -> ECB_BUS_NO_CANDIDATE; more -> ECB_BUS_AMBIGUOUS.
//      (A lane per miss would walk its 48 .. 96 lookups one behind the other -- each a dependent chain of directory read and bucket read
//      -- and its lanes would diverge in the buckets; it was not built: there is one path and no switch.)
//   3. the keep flags and the ambiguous flags scanned (the four sizes follow); || read back: the capacity.  k_busc_emit copies the kept
//      records to their places, 32 bytes each, with the barcode of a corrected one replaced (BusRec is packed: any alignment on both
//      sides).  The status bytes are the call's own until then: a refusal has written nothing.
namespace {
constexpr u32 BUSC_BUCKET_AVG = 4;                   // the directory is sized so that an average bucket holds at most this many entries
constexpr u32 BUSC_DIR_MAX_BITS = 24;                // ... with at most this many bits (2^24 + 1 offsets: 64 MB)
constexpr u32 BUSC_BISECT_LEN = 16;                  // a bucket up to this long is read whole, a longer one bisected (busc_has)
constexpr u32 BUSC_LANES = 64;                       // lanes that share a miss's neighbours: a wave
constexpr u32 BUSC_MISS = 255u;                      // the status of a record between k_busc_exact and k_busc_neigh
enum : u32 { BUSC_W_ORDER = 1, BUSC_W_BIT };
static_assert(TPB % BUSC_LANES == 0 && BUSC_LANES == 64, "a miss is a wave's work, and __ballot is 64 bits wide");

const char* busc_white_reason(u32 r) {
    switch (r) {
    case BUSC_W_ORDER: return "not above the entry before it";
    case BUSC_W_BIT: return "a bit at or above 2 x bclen";
    default: return "unknown";
    }
}
inline u32 busc_dir_bits(u64 n_white, u32 bclen) {
    u32 b = 0;
    while (b < BUSC_DIR_MAX_BITS && b < 2 * bclen && ((u64)BUSC_BUCKET_AVG << b) < n_white) ++b;
    return b;
}
// the whitelist with its directory: prefix(bc) = bits ? bc >> shift : 0, shift = 2 x bclen - bits (0 .. 63 whenever bits > 0)
struct BuscTable { const u64* white; const u32* dir; u32 bits, shift; };
__device__ __forceinline__ u64 busc_prefix(const BuscTable& t, u64 bc) { return t.bits ? bc >> t.shift : 0ull; }
// whether the whitelist holds bc (bc below 4^bclen: its prefix is below 2^bits)
__device__ __forceinline__ bool busc_has(const BuscTable& t, u64 bc) {
    const u64 p = busc_prefix(t, bc);
    u32 lo = t.dir[p], hi = t.dir[p + 1];
    if (hi - lo <= BUSC_BISECT_LEN) {
        bool found = false;
        for (u32 j = lo; j < hi; ++j) found |= t.white[j] == bc;
        return found;
    }
    const u32 end = hi;
    while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; if (t.white[mid] < bc) lo = mid + 1; else hi = mid; }
    return lo < end && t.white[lo] == bc;
}
__global__ __launch_bounds__(TPB) void k_busc_white(const u64* white, u64 n_white, u32 bcbits, u64* err) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n_white) return;
    const u64 w = white[j];
    if (j > 0 && white[j - 1] >= w) offender(err, j, BUSC_W_ORDER);
    else if (bcbits < 64u && (w >> bcbits)) offender(err, j, BUSC_W_BIT);
}
// directory entry p of 2^bits + 1
__global__ __launch_bounds__(TPB) void k_busc_dir(BuscTable t, u64 n_white, u32* dir) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x, np = 1ull << t.bits;
    if (p > np) return;
    dir[p] = p == np ? (u32)n_white : (u32)lower_bound_u64(t.white, n_white, t.bits ? p << t.shift : 0ull);
}
// record i: checked; in the whitelist or a miss
__global__ __launch_bounds__(TPB) void k_busc_exact(const BusRec* recs, u64 n, u32 bcbits, BuscTable t, u64* err, uint8_t* status, u32* miss) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u64 bc = recs[i].barcode;
    bool found = true;
    if (bcbits < 64u && (bc >> bcbits)) offender(err, i, BUS_R_BARCODE);
    else found = busc_has(t, bc);
    status[i] = found ? (uint8_t)ECB_BUS_EXACT : (uint8_t)BUSC_MISS;
    miss[i] = !found;
}
__global__ __launch_bounds__(TPB) void k_busc_list(const u32* miss, const u32* mpos, u64 n, u32* mlist) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n && miss[i]) mlist[mpos[i]] = (u32)i;
}
// one wave per miss: a neighbour per lane and round
__global__ __launch_bounds__(TPB) void k_busc_neigh(const BusRec* recs, const u32* mlist, u64 n_miss, u32 bclen, BuscTable t, uint8_t* status, u64* newbc,
                                                    u32* amb) {
    const u64 m = blockIdx.x * (u64)(TPB / BUSC_LANES) + threadIdx.x / BUSC_LANES;
    if (m >= n_miss) return;                                    // (a whole wave leaves or stays)
    const u32 lane = threadIdx.x % BUSC_LANES, nq = 3u * bclen;
    const u32 i = mlist[m];
    const u64 bc = recs[i].barcode;
    u32 total = 0;
    u64 mine = 0;
    bool mine_hit = false;
    for (u32 base = 0; base < nq; base += BUSC_LANES) {
        const u32 q = base + lane;
        bool hit = false;
        if (q < nq) {
            const u64 nb = bc ^ ((u64)(1u + q % 3u) << (2u * (q / 3u)));      // (q / 3 <= 31: a shift of 62 at the most)
            hit = busc_has(t, nb);
            if (hit) { mine = nb; mine_hit = true; }
        }
        total += (u32)__popcll(__ballot(hit));
    }
    if (total == 1u) { if (mine_hit) { newbc[m] = mine; status[i] = (uint8_t)ECB_BUS_CORRECTED; } }
    else if (lane == 0u) status[i] = total ? (uint8_t)ECB_BUS_AMBIGUOUS : (uint8_t)ECB_BUS_NO_CANDIDATE;
    if (lane == 0u) amb[m] = total > 1u;
}
__global__ __launch_bounds__(TPB) void k_busc_keep(const uint8_t* status, u64 n, u32* keep) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) keep[i] = status[i] <= ECB_BUS_CORRECTED;
}
// a kept record to its place, the barcode of a corrected one replaced; the status bytes to the caller
__global__ __launch_bounds__(TPB) void k_busc_emit(const BusRec* recs, u64 n, const uint8_t* status, const u32* kpos, const u32* mpos, const u64* newbc,
                                                   BusRec* out, uint8_t* out_status) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u32 s = status[i];
    if (out_status) out_status[i] = (uint8_t)s;
    if (s > ECB_BUS_CORRECTED) return;
    BusRec r = recs[i];
    if (s == ECB_BUS_CORRECTED) r.barcode = newbc[mpos[i]];
    out[kpos[i]] = r;
}

int busc_check_args(const void* records, uint64_t n, uint32_t bclen, const void* whitelist, uint64_t n_white, uint64_t cap_out, const void* out_records,
                    const void* out_sizes) {
    if (!records || !n || !whitelist || !n_white || !out_sizes || (cap_out && !out_records)) return fail(nullptr, ECB_ERR_ARG, "bus: bad argument");
    if (bclen < 1 || bclen > 32) return fail(nullptr, ECB_ERR_ARG, "bus: bclen is 1 .. 32");
    if (n >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "bus: 2^30 records or more");
    if (n_white >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "bus: a whitelist of 2^31 entries or more");
    if (spans_overlap({records, n * 32}, {out_records, std::min<u64>(cap_out, n) * 32}))      // (more room than n records is never written)
        return fail(nullptr, ECB_ERR_ARG, "bus: out_records overlaps records");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_bus_correct_device(int device, const void* d_records, uint64_t n, uint32_t bclen, const void* d_whitelist, uint64_t n_white,
                                      uint64_t cap_out, void* d_out_records, void* d_out_status, uint64_t* out_sizes) {
    RCCHK(busc_check_args(d_records, n, bclen, d_whitelist, n_white, cap_out, d_out_records, out_sizes));
    Call c(device, "bus: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const BusRec* recs = (const BusRec*)d_records;
    const u32 bcbits = 2 * bclen, bits = busc_dir_bits(n_white, bclen);
    const u64 n_dir = (1ull << bits) + 1;
    // [0] lowest (whitelist entry << 8 | reason)  [1] lowest (record << 8 | reason)  [2] misses  [3] records kept  [4] ambiguous
    u64* words;
    RCCHK(c.status_words(words, 8, 2));
    u32* dir = c.get<u32>(CV_X2, n_dir);
    Arena ar(c, CV_X0, Arena::pad(n, 1) + 2 * Arena::pad(n, 4) + 2 * Arena::pad(n + 1, 4) + Arena::pad(scan_words(n), 4));
    RCCHK(c.missing());
    uint8_t* status = ar.take<uint8_t>(n);
    u32 *miss = ar.take<u32>(n), *keep = ar.take<u32>(n), *mpos = ar.take<u32>(n + 1), *kpos = ar.take<u32>(n + 1), *sums = ar.take<u32>(scan_words(n));
    RCCHK(ar.missing(c));
    const BuscTable t{(const u64*)d_whitelist, dir, bits, bcbits - bits};
    u64 back[8];
    // 0. the whitelist, then its directory
    k_busc_white<<<nblk(n_white, TPB), TPB, 0, st>>>(t.white, n_white, bcbits, words);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words, 2));
    RCCHK(refuse_offender(back[0], "bus: whitelist entry", busc_white_reason));      // (the directory of a list that is not ascending would be none)
    k_busc_dir<<<nblk(n_dir, TPB), TPB, 0, st>>>(t, n_white, dir);
    // 1. the exact lookups; the misses listed
    k_busc_exact<<<nblk(n, TPB), TPB, 0, st>>>(recs, n, bcbits, t, words + 1, status, miss);
    CALLCHK(c, scan_launch(st, miss, n, mpos, sums, words + 2));
    RCCHK(c.read_back(back, words, 3));
    RCCHK(refuse_offender(back[1], "bus: record", bus_record_reason));
    const u64 n_miss = back[2];
    // 2. the neighbours of the misses
    Arena am(c, CV_X1, Arena::pad(n_miss, 8) + 2 * Arena::pad(n_miss, 4) + Arena::pad(n_miss + 1, 4) + Arena::pad(scan_words(n_miss), 4));
    RCCHK(c.missing());
    u64* newbc = am.take<u64>(n_miss);
    u32 *mlist = am.take<u32>(n_miss), *amb = am.take<u32>(n_miss), *apos = am.take<u32>(n_miss + 1), *sums2 = am.take<u32>(scan_words(n_miss));
    RCCHK(am.missing(c));
    if (n_miss) {
        k_busc_list<<<nblk(n, TPB), TPB, 0, st>>>(miss, mpos, n, mlist);
        k_busc_neigh<<<nblk(n_miss, TPB / BUSC_LANES), TPB, 0, st>>>(recs, mlist, n_miss, bclen, t, status, newbc, amb);
        CALLCHK(c, scan_launch(st, amb, n_miss, apos, sums2, words + 4));
    }
    // 3. the sizes, the capacity, then the outputs
    k_busc_keep<<<nblk(n, TPB), TPB, 0, st>>>(status, n, keep);
    CALLCHK(c, scan_launch(st, keep, n, kpos, sums, words + 3));
    RCCHK(c.read_back(back, words, 5));
    const u64 n_kept = back[3], n_amb = n_miss ? back[4] : 0, n_exact = n - n_miss, n_corr = n_kept - n_exact;
    if (n_kept > cap_out)
        return fail(nullptr, ECB_ERR_ARG, "bus: %llu records kept; room for %llu", (unsigned long long)n_kept, (unsigned long long)cap_out);
    k_busc_emit<<<nblk(n, TPB), TPB, 0, st>>>(recs, n, status, kpos, mpos, newbc, (BusRec*)d_out_records, (uint8_t*)d_out_status);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, hipStreamSynchronize(st));
    const u64 sizes[4] = {n_exact, n_corr, n_miss - n_corr - n_amb, n_amb};
    memcpy(out_sizes, sizes, sizeof sizes);
    return ECB_OK;
}

extern "C" int ecb_bus_correct(int device, const void* records, uint64_t n, uint32_t bclen, const uint64_t* whitelist, uint64_t n_white, uint64_t cap_out,
                               void* out_records, uint8_t* out_status, uint64_t* out_sizes) {
    RCCHK(busc_check_args(records, n, bclen, whitelist, n_white, cap_out, out_records, out_sizes));
    Call c(device, "bus: "); if (c.rc) return c.rc;
    const u64 room = std::min<u64>(cap_out, n);                  // (at most n records are kept: more room is never used)
    DevBuf<> dr, dw, dout, ds;
    std::vector<StageIn> in = {{&dr, records, n * 32}, {&dw, whitelist, n_white * 8}, {&dout, nullptr, room * 32}};
    if (out_status) in.push_back({&ds, nullptr, n});
    RCCHK(stage_in(c, in));
    RCCHK(ecb_bus_correct_device(device, dr.p, n, bclen, dw.p, n_white, room, dout.p, out_status ? ds.p : nullptr, out_sizes));
    return stage_out(c, {{out_records, &dout, (out_sizes[0] + out_sizes[1]) * 32}, {out_status, &ds, out_status ? n : 0}});
}
