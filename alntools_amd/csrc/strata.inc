// ---- --best-strata: of every read's passing records, the best-scoring ones kept (ecb_best_strata / ecb_best_strata_device; included by
// ecb.hip; of its siblings it needs none: Call, the lowest-offender word, tuple_step, Arena and the span check are ecb.hip's) -------------
// The rule is include/ecb_strata.h's.  A read's verdict is ONE 64-bit word, key = (biased score << 32 | record index), the minimum over
// the read's passing records (mode "highest" flips the biased score): its high word is the best score, its low word the first kept
// record; next to it travels the index of the read's first passing record, a minimum too.  Minima do not depend on arrival order.
//   A lane holds STRATA_LANE_RECS = 4 consecutive records (one 16-byte load of each stream where the pointer allows it), a wave
//   STRATA_WAVE_RECS = 256, a workgroup STRATA_WG_RECS = 1024: four waves that share nothing.
//   In a lane, the records of one read are combined in registers.  Across the wave, a read is a run of lanes: a lane's tail group (the
//   records with its last id) is scanned upwards, its head group downwards, by shuffles, the runs cut where __ballot says a lane is not
//   wholly one read that joins its neighbour (strata_wave).  What a wave cannot settle is a read that crosses its span -- at most two,
//   its first and its last: those send their word to global memory, one atomicMin each, into the slot of THE WAVE THE READ STARTS IN.
//   That wave is found by position, never by value: a gallop back from the wave's first record, then a bisection, comparing ids
//   (strata_read_start).  So no index is derived from a read_id, a malformed stream addresses nothing outside the buffers, and a
//   read of any length -- the unmapped tail of a file -- costs its waves one search and at most one atomic each (none where the wave
//   holds no passing record of it).
//   1. k_strata_reduce: 12 bytes per record in.  The contract checked against the record before (the lowest offender by an atomicMin
//      of (record << 8 | reason)); the crossing reads' words to their slots; per wave the two slots it must read again (strata info).
//      || read back: refusal.  Nothing of the caller's has been written.
//   2. k_strata_apply: 12 bytes per record in, 8 out.  The same wave reduction, the crossing reads' words taken from their slots, the
//      verdict per record, the wave's four counts by __ballot, stored per wave.  A wave reads only its own records, so an output may
//      be its input.  k_strata_sum adds the waves' counts up.  || read back: the counts.
namespace {
constexpr u32 STRATA_LANE_RECS = 4;                           // records per lane
constexpr u32 STRATA_WAVE_RECS = 64 * STRATA_LANE_RECS;       // records per wave
constexpr u32 STRATA_WG_RECS = (TPB / 64) * STRATA_WAVE_RECS; // records per workgroup
constexpr u32 STRATA_SUM_WAVES = 16;                          // waves whose counts one thread of k_strata_sum adds up
constexpr u32 STRATA_NONE = 0xFFFFFFFFu;                      // no slot: the wave's first (last) read does not cross its span
constexpr u64 STRATA_INF = ~0ull;                             // the word of a read without a passing record (no real key: n < 2^32)
constexpr u32 STRATA_DROP_BITS = 0x4u | ECB_FLAG_STRATA_DROPPED;
static_assert(STRATA_LANE_RECS == 4 && TPB % 64 == 0, "a lane's records are one 16-byte vector, a workgroup is whole waves");

// records [i, i + 4) of a stream (i a multiple of 4): one vector where the stream is 16-byte aligned and the four exist, otherwise one
// by one; a record at or beyond n reads as record n - 1
__device__ __forceinline__ void strata_load(const u32* p, bool vec, u64 i, u64 n, u32 (&v)[STRATA_LANE_RECS]) {
    if (vec && i + STRATA_LANE_RECS <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (u32 q = 0; q < STRATA_LANE_RECS; ++q) v[q] = p[i + q < n ? i + q : n - 1];
    }
}
__device__ __forceinline__ void strata_store(u32* p, bool vec, u64 i, u64 n, const u32 (&v)[STRATA_LANE_RECS]) {
    if (vec && i + STRATA_LANE_RECS <= n) *reinterpret_cast<uint4*>(p + i) = make_uint4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (u32 q = 0; q < STRATA_LANE_RECS; ++q) if (i + q < n) p[i + q] = v[q];
    }
}
__device__ __forceinline__ bool strata_vec(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// a lane's four records: ids counted from the stream's first (they never fall in a stream that obeys the contract), the filter's
// verdict, the key and the first-passing candidate of each
struct StrataLane {
    u32 id[STRATA_LANE_RECS], hf[STRATA_LANE_RECS], rel[STRATA_LANE_RECS], fp[STRATA_LANE_RECS];
    u64 key[STRATA_LANE_RECS];
    bool pass[STRATA_LANE_RECS];
};
__device__ __forceinline__ void strata_lane(const u32* rid, const u32* hf, const u32* score, u64 i, u64 n, u32 flip, StrataLane& a) {
    u32 sc[STRATA_LANE_RECS];
    const u32 id0 = rid[0];
    strata_load(rid, strata_vec(rid), i, n, a.id);
    strata_load(hf, strata_vec(hf), i, n, a.hf);
    strata_load(score, strata_vec(score), i, n, sc);
#pragma unroll
    for (u32 q = 0; q < STRATA_LANE_RECS; ++q) {
        a.rel[q] = a.id[q] - id0;
        a.pass[q] = i + q < n && rec_valid(a.hf[q]);
        a.fp[q] = a.pass[q] ? (u32)(i + q) : STRATA_NONE;
        a.key[q] = a.pass[q] ? (u64)((sc[q] ^ 0x80000000u) ^ flip) << 32 | (u32)(i + q) : STRATA_INF;     // (a score is looked at in a passing record only)
    }
}
// the wave's reduction: K[q], P[q] = the minima over the records of THIS WAVE that share record q's id
__device__ __forceinline__ void strata_wave(const StrataLane& a, u32 lane, u64 (&K)[STRATA_LANE_RECS], u32 (&P)[STRATA_LANE_RECS]) {
#pragma unroll
    for (u32 q = 0; q < STRATA_LANE_RECS; ++q) {
        K[q] = a.key[q]; P[q] = a.fp[q];
#pragma unroll
        for (u32 r = 0; r < STRATA_LANE_RECS; ++r)
            if (a.rel[r] == a.rel[q]) { K[q] = min(K[q], a.key[r]); P[q] = min(P[q], a.fp[r]); }
    }
    const u32 first = a.rel[0], last = a.rel[STRATA_LANE_RECS - 1];
    const bool whole = first == last;
    const u32 below = __shfl_up(last, 1), above = __shfl_down(first, 1);      // (every lane takes part: not behind the && below)
    const bool joins_left = lane > 0 && below == first, joins_right = lane < 63 && above == last;
    // a run of the upward scan begins at a lane that is not wholly its left neighbour's read; of the downward one, likewise to the right
    const u64 heads = __ballot(!(whole && joins_left)), tails = __ballot(!(whole && joins_right));
    const u32 s = 63u - (u32)__clzll(heads & (~0ull >> (63u - lane)));       // (lane 0 is a head, lane 63 a tail: both exist)
    const u32 e = lane + (u32)__ffsll(tails >> lane) - 1u;
    u64 uk = K[STRATA_LANE_RECS - 1], dk = K[0];
    u32 up = P[STRATA_LANE_RECS - 1], dp = P[0];
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const u64 ok = __shfl_up(uk, d), pk = __shfl_down(dk, d);
        const u32 op = __shfl_up(up, d), pp = __shfl_down(dp, d);
        if (lane >= s + d) { uk = min(uk, ok); up = min(up, op); }
        if (lane + d <= e) { dk = min(dk, pk); dp = min(dp, pp); }
    }
    // the records below this lane with its first id, and those above it with its last
    u64 lk = __shfl_up(uk, 1), rk = __shfl_down(dk, 1);
    u32 lp = __shfl_up(up, 1), rp = __shfl_down(dp, 1);
    if (!joins_left) { lk = STRATA_INF; lp = STRATA_NONE; }
    if (!joins_right) { rk = STRATA_INF; rp = STRATA_NONE; }
#pragma unroll
    for (u32 q = 0; q < STRATA_LANE_RECS; ++q) {
        if (a.rel[q] == first) { K[q] = min(K[q], lk); P[q] = min(P[q], lp); }
        if (a.rel[q] == last) { K[q] = min(K[q], rk); P[q] = min(P[q], rp); }
    }
}
// the first record of the read that record s - 1 belongs to (its id, counted from the stream's first, is x): the lowest p of [0, s) with
// rid[p] - id0 >= x.  A gallop back -- a short read is found in a step or two, in the line the wave before has just read --, then a
// bisection.  Every index lies in [0, s): on a stream that does not obey the contract the answer is some record, and nothing else
__device__ __forceinline__ u64 strata_read_start(const u32* rid, u32 id0, u64 s, u32 x) {
    u64 right = s - 1, left = 0, step = 1;                   // rid[right] - id0 >= x; everything below `left` is below x
    for (;;) {
        if (step > right) break;
        const u64 q = right - step;
        if (rid[q] - id0 < x) { left = q + 1; break; }
        right = q; step *= 2;
    }
    while (left < right) { const u64 mid = left + (right - left) / 2; if (rid[mid] - id0 >= x) right = mid; else left = mid + 1; }
    return left;
}
__global__ __launch_bounds__(TPB) void k_strata_reduce(const u32* rid, const u32* hf, const u32* score, u64 n, u32 flip, u64* err, u64* best,
                                                       u32* firstp, u32* info) {
    const u64 w = blockIdx.x * (u64)(TPB / 64) + threadIdx.x / 64, base = w * STRATA_WAVE_RECS;
    if (base >= n) return;                                    // (a whole wave leaves or stays)
    const u32 lane = threadIdx.x % 64;
    const u64 i = base + (u64)lane * STRATA_LANE_RECS;
    StrataLane a;
    strata_lane(rid, hf, score, i, n, flip, a);
    // the contract, record by record against the one before (record 0 has none: its id may be anything)
    u32 prev = __shfl_up(a.id[STRATA_LANE_RECS - 1], 1);
    if (lane == 0) prev = base ? rid[base - 1] : a.id[0];
    const u32 left = prev;
#pragma unroll
    for (u32 q = 0; q < STRATA_LANE_RECS; ++q) {
        const u32 why = i + q < n ? tuple_step(prev, a.id[q], a.pass[q]) : 0u;
        if (why) offender(err, i + q, why);
        prev = a.id[q];
    }
    u64 K[STRATA_LANE_RECS];
    u32 P[STRATA_LANE_RECS];
    strata_wave(a, lane, K, P);
    // the reads that cross the wave's span: the first one to the slot of the wave it starts in, the last one to this wave's -- or, where
    // the whole wave is one read that began before it, to that same slot, once
    const u64 end = base + STRATA_WAVE_RECS;
    u32 hs = STRATA_NONE;
    if (lane == 0 && base && left == a.id[0]) {
        hs = (u32)(strata_read_start(rid, rid[0], base, a.rel[0]) / STRATA_WAVE_RECS);
        if (K[0] != STRATA_INF) atomicMin(reinterpret_cast<unsigned long long*>(best + hs), (unsigned long long)K[0]);
        if (P[0] != STRATA_NONE) atomicMin(firstp + hs, P[0]);
    }
    hs = __shfl(hs, 0);
    const bool one_read = __shfl(a.rel[0], 0) == __shfl(a.rel[STRATA_LANE_RECS - 1], 63);
    if (lane == 0) info[2 * w] = hs;
    if (lane == 63) {
        u32 ts = STRATA_NONE;
        if (end < n && rid[end] == a.id[STRATA_LANE_RECS - 1]) {
            if (one_read && hs != STRATA_NONE) ts = hs;
            else {
                ts = (u32)w;
                if (K[STRATA_LANE_RECS - 1] != STRATA_INF) atomicMin(reinterpret_cast<unsigned long long*>(best + ts), (unsigned long long)K[STRATA_LANE_RECS - 1]);
                if (P[STRATA_LANE_RECS - 1] != STRATA_NONE) atomicMin(firstp + ts, P[STRATA_LANE_RECS - 1]);
            }
        }
        info[2 * w + 1] = ts;
    }
}
__global__ __launch_bounds__(TPB) void k_strata_apply(const u32* rid, const u32* hf, const u32* score, u64 n, u32 flip, const u64* best,
                                                      const u32* firstp, const u32* info, u32* out_rid, u32* out_hf, u32* wcount) {
    const u64 w = blockIdx.x * (u64)(TPB / 64) + threadIdx.x / 64, base = w * STRATA_WAVE_RECS;
    if (base >= n) return;
    const u32 lane = threadIdx.x % 64;
    const u64 i = base + (u64)lane * STRATA_LANE_RECS;
    StrataLane a;
    strata_lane(rid, hf, score, i, n, flip, a);
    u64 K[STRATA_LANE_RECS];
    u32 P[STRATA_LANE_RECS];
    strata_wave(a, lane, K, P);
    const u32 hs = info[2 * w], ts = info[2 * w + 1];
    const u32 first = __shfl(a.rel[0], 0), last = __shfl(a.rel[STRATA_LANE_RECS - 1], 63);
    const u64 hk = hs != STRATA_NONE ? best[hs] : STRATA_INF, tk = ts != STRATA_NONE ? best[ts] : STRATA_INF;
    const u32 hp = hs != STRATA_NONE ? firstp[hs] : STRATA_NONE, tp = ts != STRATA_NONE ? firstp[ts] : STRATA_NONE;
    u32 oid[STRATA_LANE_RECS], ohf[STRATA_LANE_RECS];
    u32 c_pass = 0, c_kept = 0, c_drop = 0, c_first = 0;
#pragma unroll
    for (u32 q = 0; q < STRATA_LANE_RECS; ++q) {
        if (hs != STRATA_NONE && a.rel[q] == first) { K[q] = hk; P[q] = hp; }       // (the slot holds this wave's share too)
        if (ts != STRATA_NONE && a.rel[q] == last) { K[q] = tk; P[q] = tp; }
        const u32 idx = (u32)(i + q);
        const bool kept = a.pass[q] && (u32)(a.key[q] >> 32) == (u32)(K[q] >> 32), dropped = a.pass[q] && !kept;
        ohf[q] = dropped ? a.hf[q] | STRATA_DROP_BITS : a.hf[q];
        oid[q] = K[q] != STRATA_INF && idx < (u32)K[q] ? a.id[q] - 1u : a.id[q];     // before the read's first kept record
        c_pass += (u32)__popcll(__ballot(a.pass[q]));
        c_kept += (u32)__popcll(__ballot(kept));
        c_drop += (u32)__popcll(__ballot(dropped));
        c_first += (u32)__popcll(__ballot(dropped && idx == P[q]));
    }
    strata_store(out_rid, strata_vec(out_rid), i, n, oid);
    strata_store(out_hf, strata_vec(out_hf), i, n, ohf);
    if (lane < 4) wcount[4 * w + lane] = lane == 0 ? c_pass : lane == 1 ? c_kept : lane == 2 ? c_drop : c_first;
}
// the waves' four counts added up: STRATA_SUM_WAVES waves per thread, a wave's sums by shuffles, then one atomicAdd per wave and count
// (integers: any order gives the same sum).  A wave of k_strata_apply adding its own counts to the four words would be 4 atomics on one
// line per 256 records: at config 3's size 51 M of them, one behind the other -- measured, the call took 171 ms that way
__global__ __launch_bounds__(TPB) void k_strata_sum(const uint4* wcount, u64 n_waves, u64* counts) {
    u64 c[4] = {0, 0, 0, 0};
    for (u32 k = 0; k < STRATA_SUM_WAVES; ++k) {
        const u64 w = (blockIdx.x * (u64)STRATA_SUM_WAVES + k) * TPB + threadIdx.x;
        if (w < n_waves) { const uint4 v = wcount[w]; c[0] += v.x; c[1] += v.y; c[2] += v.z; c[3] += v.w; }
    }
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        for (u32 d = 32; d; d >>= 1) c[q] += __shfl_down(c[q], d);
        if (threadIdx.x % 64 == 0 && c[q]) atomicAdd(reinterpret_cast<unsigned long long*>(counts + q), c[q]);
    }
}

int strata_check_args(const void* read_id, const void* hapflag, const void* score, uint64_t n, uint32_t mode, const void* out_read_id,
                      const void* out_hapflag, const void* out_counts) {
    if (!read_id || !hapflag || !score || !out_read_id || !out_hapflag || !out_counts || !n) return fail(nullptr, ECB_ERR_ARG, "strata: bad argument");
    if (mode != ECB_STRATA_LOWEST && mode != ECB_STRATA_HIGHEST) return fail(nullptr, ECB_ERR_ARG, "strata: mode is 0 (lowest) or 1 (highest)");
    if (n >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "strata: 2^32 records or more");
    const u64 bytes = n * 4;
    const std::vector<Span> spans = {{read_id, bytes}, {hapflag, bytes}, {score, bytes}, {out_read_id, bytes}, {out_hapflag, bytes}};
    for (const Span& s : spans) if ((uintptr_t)s.p & 3u) return fail(nullptr, ECB_ERR_ARG, "strata: a pointer that is not 4-byte aligned");
    // an output may be exactly its own input; any other two of the five that an output is one of may not share a byte
    if (span_clash(spans, 2, {0, 1}))
        return fail(nullptr, ECB_ERR_ARG, "strata: an output overlaps an input or the other output (it may only be exactly its own input)");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_best_strata_device(int device, const void* d_read_id, const void* d_hapflag, const void* d_score, uint64_t n, uint32_t mode,
                                      void* d_out_read_id, void* d_out_hapflag, uint64_t* out_counts) {
    RCCHK(strata_check_args(d_read_id, d_hapflag, d_score, n, mode, d_out_read_id, d_out_hapflag, out_counts));
    Call c(device, "strata: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 n_waves = (n + STRATA_WAVE_RECS - 1) / STRATA_WAVE_RECS;
    u64* words;                                              // [0] lowest (record << 8 | reason)  [1 .. 4] the counts
    RCCHK(c.status_words(words, 8, 1));
    Arena ar(c, CV_X0, Arena::pad(n_waves, 8) + Arena::pad(n_waves, 4) + Arena::pad(2 * n_waves, 4) + Arena::pad(4 * n_waves, 4));
    RCCHK(c.missing());
    u64* best = ar.take<u64>(n_waves);
    u32 *firstp = ar.take<u32>(n_waves), *info = ar.take<u32>(2 * n_waves), *wcount = ar.take<u32>(4 * n_waves);
    RCCHK(ar.missing(c));
    const u32 flip = mode == ECB_STRATA_HIGHEST ? 0xFFFFFFFFu : 0u;
    const u32 *rid = (const u32*)d_read_id, *hf = (const u32*)d_hapflag, *sc = (const u32*)d_score;
    u64 back[8];
    CALLCHK(c, hipMemsetAsync(best, 0xFF, Arena::pad(n_waves, 8) + Arena::pad(n_waves, 4), st));      // (best and firstp lie behind each other)
    k_strata_reduce<<<nblk(n, STRATA_WG_RECS), TPB, 0, st>>>(rid, hf, sc, n, flip, words, best, firstp, info);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words, 1));
    RCCHK(refuse_offender(back[0], "strata: record", tuple_reason));
    k_strata_apply<<<nblk(n, STRATA_WG_RECS), TPB, 0, st>>>(rid, hf, sc, n, flip, best, firstp, info, (u32*)d_out_read_id, (u32*)d_out_hapflag, wcount);
    k_strata_sum<<<nblk(n_waves, STRATA_SUM_WAVES * TPB), TPB, 0, st>>>(reinterpret_cast<const uint4*>(wcount), n_waves, words + 1);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words + 1, 4));
    memcpy(out_counts, back, 4 * 8);
    return ECB_OK;
}

extern "C" int ecb_best_strata(int device, const uint32_t* read_id, const uint32_t* hapflag, const int32_t* score, uint64_t n, uint32_t mode,
                               uint32_t* out_read_id, uint32_t* out_hapflag, uint64_t* out_counts) {
    RCCHK(strata_check_args(read_id, hapflag, score, n, mode, out_read_id, out_hapflag, out_counts));
    Call c(device, "strata: "); if (c.rc) return c.rc;
    DevBuf<> di, df, ds, oi, of;
    RCCHK(stage_in(c, {{&di, read_id, n * 4}, {&df, hapflag, n * 4}, {&ds, score, n * 4}, {&oi, nullptr, n * 4}, {&of, nullptr, n * 4}}));
    RCCHK(ecb_best_strata_device(device, di.p, df.p, ds.p, n, mode, oi.p, of.p, out_counts));
    return stage_out(c, {{out_read_id, &oi, n * 4}, {out_hapflag, &of, n * 4}});
}
