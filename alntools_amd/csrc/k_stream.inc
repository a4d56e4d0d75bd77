// k_stream and what depends on its pass geometry: compiled twice by ecb.hip (namespace ks_std: passes of up to 64 reads, five waves per SIMD;
// namespace ks_short, ECB_KS_SHORT 1: passes of up to 128 reads in a table twice the size with one-byte masks, four waves per SIMD -- streams of short reads,
// where a 512-record tile holds more reads than a pass of 64 takes and every further visit of the tile costs the filter and the LDS inserts again).
// Not a translation unit of its own.
constexpr bool KS_SHORT = ECB_KS_SHORT != 0;
#ifndef ECB_KS_PAR
#define ECB_KS_PAR 0
#endif
// namespace ks_par, ECB_KS_PAR 1: ks_std with the key compare that settles displaced pairs in registers (LdsSetCmp::quick) -- for streams whose reads
// hit loci anywhere among the targets (paralogs), where every tile has records that find their first slot taken and every flush a read whose
// key holds such a pair.  The library counts the tiles that take the probe-on path and picks this compilation for the batches after one in
// which more than a quarter did (process_batch); the plain compilations keep round 3's short compare, which costs them nothing.
constexpr bool KS_PAR = ECB_KS_PAR != 0;
static_assert(!(KS_PAR && KS_SHORT), "one or the other");
constexpr u32 KBITS = KS_SHORT ? 25 : 26;          // LDS keys: locus + 1 in the low KBITS bits, the read's index within the pass above them
constexpr u32 KMASK = (1u << KBITS) - 1u;
constexpr int WMAXR = KS_SHORT ? 128 : 64;      // reads a pass takes at most (phase (c): one lane each, in rounds of 64)
#ifndef ECB_WAVES_PER_SIMD
#define ECB_WAVES_PER_SIMD 5   // 96 VGPRs, 7.4 KB of LDS per wave: five workgroups per CU (measured against four with 128 / 9.4 KB: -7.5 % on C3)
#endif
#ifndef ECB_LGMAX
#define ECB_LGMAX 6            // a pass takes at most 1 << ECB_LGMAX reads (one lane each in phase (c): 6 at most)
#endif
#ifndef ECB_EST_MUL
#define ECB_EST_MUL 4          // ... and is laid out for this many tiles like the one that ended the pass before
#endif
constexpr int WAVES_PER_SIMD = KS_SHORT ? 4 : ECB_WAVES_PER_SIMD;   // (short reads: 9.9 KB of LDS per wave -- the masks are bytes there: at most 8 haplotypes)
constexpr int LGMAX = KS_SHORT ? 7 : ECB_LGMAX;
static_assert(LGMAX >= 0 && (1 << LGMAX) <= WMAXR && KBITS + LGMAX <= 32, "a read's index within the pass: the bits of an LDS key above KBITS");
constexpr int CMAX = KS_SHORT ? 64 : 80;              // (locus, mask) entries an unfinished read may carry into the next tile
#ifndef ECB_TSLOTS
#define ECB_TSLOTS (ECB_WAVES_PER_SIMD > 4 ? 640 : 896)
#endif
constexpr int TSLOTS = KS_SHORT ? 1280 : ECB_TSLOTS;  // LDS table slots per wave and pass (at most WT + CMAX = 592 entries): 1.75 or 1.25 x 512; 128 reads: 2.5 x 512
constexpr int TBASE = KS_SHORT ? 1024 : 512;          // slots shared out as home regions: a read of nb gets TBASE >> ceil(log2 nb) of them (+ a quarter or three quarters)
constexpr int TAB_BYTES = KS_SHORT ? TSLOTS * 4 + 2048 : TSLOTS * 8;      // keys + masks (128 reads: a byte per mask, padded)
static_assert((TSLOTS == 896 || TSLOTS == 640 || TSLOTS == 1280) && WT + CMAX < TSLOTS && TAB_BYTES % (16 * 64) == 0 && (!KS_SHORT || TSLOTS <= 2048), "home regions / a free slot / clear loop");
constexpr u32 SBITS = KS_SHORT ? 11 : 10;             // bits of a table-slot index
constexpr u32 SMASK = (1u << SBITS) - 1u;
static_assert(TSLOTS <= (1 << SBITS) && (KS_SHORT || SBITS + LGMAX <= 16), "ent[] packs slot | read << SBITS into 16 bits (128 reads: the slot alone, the read is in the table's key)");
struct alignas(16) WaveLds {
    // ONE {(read, locus) -> haplotype mask} table for the reads of a pass: key = locus + 1 | read index << KBITS, mask = OR of
    // haplotype bits.  Read r of nb probes from r * G' + (key & (G - 1)), G = 512 >> ceil(log2 nb), G' = 1.75 G: the loci of a
    // read are mostly consecutive target ids, which the low bits never collide on, the reads' home regions are disjoint, and a
    // read with more loci than its region simply probes on into its neighbour's (the keys say whose an entry is).  The geometry
    // is two wave-uniform numbers; per-read extents (a scatter of head positions through LDS, a repack, a gather per record) were
    // a fifth of the kernel's instructions.
    // Two arrays, not one of pairs: at an 8-byte stride the compare-and-swaps of a wave land on the even banks only.
#ifdef ECB_TAB_INTERLEAVED
    uint2 tab[TSLOTS];
#else
    u32 tkey[TSLOTS];
    u32 tmask[KS_SHORT ? 512 : TSLOTS];   // (contiguous with tkey: cleared together with 16-byte stores)  128 reads: one BYTE per slot, four to a word (and the
                                     //  two arrays padded to a multiple of the clear loop's 1 KB)
#endif
    u64 acc[WMAXR];                  // per read: set-hash sum
    uint2 carry[CMAX];               // the entries of the read that is still open at the end of a tile (x = locus + 1, y = mask)
    unsigned short ent[WT + CMAX];   // table entries created in this pass: slot | read << SBITS
    unsigned short npair[WMAXR];     // per read: number of (locus, mask) pairs
    u32 ws[8];                       // wave scalars that are touched once in a while (scalar registers are scarcer than the few LDS reads):
};                                   //   [0,1] head record of the open read   [2,3] key-arena reservation: next pair   [4] ... pairs left   [5,6] where a park resumes
static_assert(sizeof(WaveLds) * NWAVE * WAVES_PER_SIMD <= 160 * 1024, "WAVES_PER_SIMD workgroups per CU");
__device__ __forceinline__ u64 ws_get64(const WaveLds& L, int i) {
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)L.ws[i]), hi = (u32)__builtin_amdgcn_readfirstlane((int)L.ws[i + 1]);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ void ws_put64(WaveLds& L, int i, u64 v, u32 lane) { if (lane == 0) { L.ws[i] = (u32)v; L.ws[i + 1] = (u32)(v >> 32); } }
#ifdef ECB_TAB_INTERLEAVED
__device__ __forceinline__ u32* tab_key(WaveLds& L, u32 q) { return &L.tab[q].x; }
__device__ __forceinline__ void tab_or(WaveLds& L, u32 q, u32 bits) { static_assert(!KS_SHORT, "byte masks: split arrays only"); atomicOr(&L.tab[q].y, bits); }
__device__ __forceinline__ uint2 tab_get(const WaveLds& L, u32 q) { return L.tab[q]; }
__device__ __forceinline__ uint4* tab_base(WaveLds& L) { return reinterpret_cast<uint4*>(L.tab); }
#else
__device__ __forceinline__ u32* tab_key(WaveLds& L, u32 q) { return &L.tkey[q]; }
__device__ __forceinline__ void tab_or(WaveLds& L, u32 q, u32 bits) {
    if constexpr (KS_SHORT) atomicOr(&L.tmask[q >> 2], bits << ((q & 3u) * 8u)); else atomicOr(&L.tmask[q], bits);
}
__device__ __forceinline__ uint2 tab_get(const WaveLds& L, u32 q) {
    if constexpr (KS_SHORT) return make_uint2(L.tkey[q], (L.tmask[q >> 2] >> ((q & 3u) * 8u)) & 0xFFu);
    else return make_uint2(L.tkey[q], L.tmask[q]);
}
__device__ __forceinline__ uint4* tab_base(WaveLds& L) { return reinterpret_cast<uint4*>(L.tkey); }
#endif
// A locus's place within its read's home region of G = 1 << g slots: bits [16, 16 + g) of locus' * fmul, fmul = 2^16 (1 + 1/G + 1/G^2 + ...) --
// that is (t + t / G + t / G^2 + ...) mod G up to rounding: consecutive target ids still land on consecutive places (a step is 1, now and
// then 2: a run of seven never meets itself at G = 8), and loci a power of two apart -- which share their low bits, so that t mod G put
// them all in one place and sent every tile of such a stream through the probe-on path (round 3: `c3s`, `c3q` at 0.37 / 0.43 of peak
// against 0.6) -- are spread by the terms above.  One 24-bit multiply and one bit-field extract per record instead of one AND.
struct HomeGeo { u32 fmul, g; };                 // (fmul: the factor in its low 24 bits -- what v_mul_u32_u24 reads; the bits above are ignored)
// The factor is worked out where the pass's geometry is chosen (once per flush) and travels with it in one word, `lgf` = factor | lg << 24:
// per tile it cost a dozen scalar instructions, and the scalar unit is shared by the CU's four SIMDs.
__device__ __forceinline__ u32 pack_lgf(u32 lg) {
    const u32 g = (u32)(KS_SHORT ? 10 : 9) - lg;       // TBASE >> lg slots, at least 8
    u32 x = 1u << 16, f = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { f += x; x >>= g; }    // (16 / 3 + 1 terms at most; below 2^24)
    return f | (lg << 24);
}
__device__ __forceinline__ HomeGeo home_geo(u32 lgf) {
    HomeGeo H;
    H.fmul = lgf;
    H.g = (u32)(KS_SHORT ? 10 : 9) - (lgf >> 24);
    return H;
}
__device__ __forceinline__ u32 home_off(u32 key, const HomeGeo& H) { return __builtin_amdgcn_ubfe(__umul24(key, H.fmul), 16u, H.g); }
// Where a key goes when its first slot (home region + the place above) is taken by another key: a second start anywhere in the
// table, then steps of a key-dependent stride that is coprime to the table size -- double hashing.  (Walking on slot by slot
// from the first probe made a tile with one read of several hundred distinct loci quadratic: its entries filled its
// neighbours' regions in one long run.)  it = probes made so far beyond the first.
__device__ __forceinline__ u32 next_slot(u32 key, u32 q, u32 it) {
    if (it == 0u) return __umulhi(key * 0x9E3779B1u, (u32)TSLOTS);
    constexpr u32 ODD_FACTOR = TSLOTS == 896 ? 7u : 5u;            // 640 = 2^7 x 5, 1280 = 2^8 x 5, 896 = 2^7 x 7
    u32 s = 1u + 2u * ((key >> 5) & 31u);
    if (s % ODD_FACTOR == 0u) s += 2u;
    q += s;
    return q >= (u32)TSLOTS ? q - (u32)TSLOTS : q;
}
// ... the same sequence in closed form: the slot of probe number `it` beyond the first (what next_slot reaches after it + 1 calls)
__device__ __forceinline__ u32 probe_slot(u32 key, u32 it) {
    u32 q = __umulhi(key * 0x9E3779B1u, (u32)TSLOTS);
    if (it != 0u) {
        constexpr u32 ODD_FACTOR = TSLOTS == 896 ? 7u : 5u;
        u32 s = 1u + 2u * ((key >> 5) & 31u);
        if (s % ODD_FACTOR == 0u) s += 2u;
        q = (q + it * s) % (u32)TSLOTS;
    }
    return q;
}

// "is the key of this slot the target set of my read?" -- the read's set is what the pass's LDS table holds under its tag,
// probed from home + home_off(key) exactly as phase (b) inserted it.  Both sides hold distinct loci, so equal sizes and every
// stored pair found with the same mask means the sets are equal.
struct LdsSetCmp {
    const WaveLds* L;
    u32 home, tag, np;               // first slot of the read's home region, read index << KBITS, number of pairs
    HomeGeo H;                       // (a locus's place within the home region)
    const StreamCold* cold;          // (the key arena, for keys longer than a slot: looked up when one turns up)
    // is (locus, mask) in my set?  The probe sequence of phase (b), from the start.
    __device__ __forceinline__ bool has(uint2 pr) const {
        const u32 key = tag | (pr.x + 1u);
        u32 q = home + home_off(pr.x + 1u, H);
        for (u32 it = 0; it < (u32)TSLOTS; ++it) {       // (the table always has a free slot)
            const uint2 t = tab_get(*L, q);
            if (t.x == key) return t.y == pr.y;
            if (t.x == 0u) return false;
            q = next_slot(key, q, it);
        }
        return false;
    }
    // On the line a lookup has just loaded.  Decides for good whenever the key is complete (CMP_EQUAL / CMP_DIFFERENT), from the registers
    // that hold the line and this wave's LDS: a locus of mine that found its first place taken is looked for at its second place -- all such
    // pairs in one more LDS round trip -- and only beyond that by the walk; the pairs of a long key come from the arena four at a time.
    // (Until round 4 a displaced pair sent the lane to table_settle -- a memory-side poll of the slot, then the key read again pair by pair,
    //  a dependent global load each: with loci anywhere among the targets, `c3r`, most flushes had such a lane and the table side of the
    //  kernel cost 5 ms instead of 1.4.)
    // The short form (round 3's; ks_std and ks_short): whatever is not in its first place is left to full(), behind table_settle.  On streams
    // whose loci sit where they probe first -- consecutive target ids, the BASELINE configs -- nothing ever is, and the longer form below,
    // compiled into the same kernel, cost config 2 three per cent and the short-read stream ten in scalar spills alone
    // (profiles/r04_ab_kvariants.txt): it lives in a compilation of its own (ks_par).
    __device__ __forceinline__ int quick_lean(const SlotView& v) const {
        if (v.n != np) return CMP_DIFFERENT;
        uint2 t[INL];                                    // the INL first probes are issued together: one LDS round trip for the lot
#pragma unroll
        for (u32 i = 0; i < INL; ++i) t[i] = tab_get(*L, i < v.n ? home + home_off(v.p[i].x + 1u, H) : home);
        bool eq = true;
#pragma unroll
        for (u32 i = 0; i < INL; ++i) eq &= i >= v.n || (t[i].x == (tag | (v.p[i].x + 1u)) && t[i].y == v.p[i].y);
        if (eq && v.n <= INL) return CMP_EQUAL;          // (the common end: every stored pair sits where its locus probes first, same mask)
        if (!eq) {                                       // rare: a mask not written yet, a locus that probed on, or another key altogether
#pragma unroll
            for (u32 i = 0; i < INL; ++i) if (i < v.n && v.p[i].y == 0u) return CMP_INCOMPLETE;
#pragma unroll
            for (u32 i = 0; i < INL; ++i)
                if (i < v.n && (t[i].x == 0u || (t[i].x == (tag | (v.p[i].x + 1u)) && t[i].y != v.p[i].y))) return CMP_DIFFERENT;   // certainly not in my set
            return CMP_UNSURE;                           // something else sits at the first probe: full() walks on
        }
        for (u32 i = INL; i < v.n; ++i) {                // the rest of a long key, from the arena
            const uint2 pr = unpack2(__hip_atomic_load(reinterpret_cast<u64*>(cold->arena + (u64)v.off + (i - INL)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (pr.y == 0u) return CMP_INCOMPLETE;
            const uint2 tt = tab_get(*L, home + home_off(pr.x + 1u, H));
            if (tt.x == (tag | (pr.x + 1u)) && tt.y == pr.y) continue;
            return (tt.x == 0u || tt.x == (tag | (pr.x + 1u))) ? CMP_DIFFERENT : CMP_UNSURE;
        }
        return CMP_EQUAL;
    }
    __device__ __forceinline__ int quick(const SlotView& v) const {
        if constexpr (!KS_PAR) return quick_lean(v);
        if (v.n != np) return CMP_DIFFERENT;
        uint2 t[INL];                                    // the INL first probes are issued together: one LDS round trip for the lot
#pragma unroll
        for (u32 i = 0; i < INL; ++i) t[i] = tab_get(*L, i < v.n ? home + home_off(v.p[i].x + 1u, H) : home);
        bool eq = true;
#pragma unroll
        for (u32 i = 0; i < INL; ++i) eq &= i >= v.n || (t[i].x == (tag | (v.p[i].x + 1u)) && t[i].y == v.p[i].y);
        if (eq && v.n <= INL) return CMP_EQUAL;          // (the common end: every stored pair sits where its locus probes first, same mask)
        // Not so: a mask not written yet, another key altogether, or a locus of mine that found its first place taken.  (The verdicts are
        // gathered in lane-local words and branched on once: a `return` per pair cost an exec mask apiece, and scalar registers are what
        // this kernel spills.)
        u32 inc = 0, diff = 0, moved = 0;                // a mask still zero / certainly not in my set / ANOTHER (read, locus) sits at the pair's first place
        if (!eq) {
#pragma unroll
        for (u32 i = 0; i < INL; ++i) {
            const u32 want = tag | (v.p[i].x + 1u);
            const u32 valid = i < v.n ? 1u : 0u, same = t[i].x == want ? 1u : 0u, none = t[i].x == 0u ? 1u : 0u;
            inc |= valid & (v.p[i].y == 0u ? 1u : 0u);
            diff |= valid & (none | (same & (t[i].y != v.p[i].y ? 1u : 0u)));
            moved |= (valid & (same ^ 1u) & (none ^ 1u)) << i;
        }
        }
        if (inc) return CMP_INCOMPLETE;
        if (diff) return CMP_DIFFERENT;
        if (moved) {                                     // a locus of mine that found its first place taken: its second place -- all such pairs in one more round trip
#pragma unroll
            for (u32 i = 0; i < INL; ++i) {
                const u32 q2 = probe_slot(tag | (v.p[i].x + 1u), 0u);
                t[i] = tab_get(*L, (moved >> i & 1u) ? q2 : home);
            }
            u32 far = 0;                                 // ... and not at their second place either
#pragma unroll
            for (u32 i = 0; i < INL; ++i) {
                const u32 want = tag | (v.p[i].x + 1u);
                const u32 m = moved >> i & 1u, same = t[i].x == want ? 1u : 0u, none = t[i].x == 0u ? 1u : 0u;
                diff |= m & (none | (same & (t[i].y != v.p[i].y ? 1u : 0u)));
                far |= (m & (same ^ 1u) & (none ^ 1u)) << i;
            }
            if (diff) return CMP_DIFFERENT;
            while (far) {                                // (rare: one copy of the walk for whichever pair it is)
                const u32 i = (u32)__builtin_ctz(far);
                far &= far - 1u;
                uint2 pr = v.p[0];
#pragma unroll
                for (u32 k = 1; k < INL; ++k) if (i == k) pr = v.p[k];
                if (!has(pr)) return CMP_DIFFERENT;
            }
        }
        for (u32 i0 = INL; i0 < v.n; i0 += 4u) {         // the rest of a long key, from the arena: four loads in flight
            u64 w[4];
#pragma unroll
            for (u32 k = 0; k < 4u; ++k)
                w[k] = __hip_atomic_load(reinterpret_cast<u64*>(cold->arena + (u64)v.off + (min(i0 + k, v.n - 1u) - INL)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (u32 k = 0; k < 4u && i0 + k < v.n; ++k) {
                const uint2 pr = unpack2(k == 0u ? w[0] : k == 1u ? w[1] : k == 2u ? w[2] : w[3]);
                if (pr.y == 0u) return CMP_INCOMPLETE;
                if (pr.x >= KMASK || !has(pr)) return CMP_DIFFERENT;     // (no read of this kernel holds such a locus)
            }
        }
        return CMP_EQUAL;                                // (every stored pair sits in my set with the same mask, and the sizes agree)
    }
    // ... on the key itself, read fresh (table_settle, behind a poll: the line showed a key still being written)
    // (its own copy of the walk, as it always was: sharing has() with quick() cost the plain compilations a third more scalar spills)
    __device__ __forceinline__ int full(Slot* s, u32 n, u32 off) const {
        if (n != np) return CMP_DIFFERENT;
        for (u32 i = 0; i < n; ++i) {
            uint2 pr = i < INL ? s->pair[i] : cold->arena[(u64)off + (i - INL)];      // (plain first: a mask that shows is final)
            if (pr.y == 0u) pr = key_pair_fresh(s, cold->arena, off, i);
            if (pr.y == 0u) return CMP_INCOMPLETE;
            if (pr.x >= KMASK) return CMP_DIFFERENT;     // (no read of this kernel holds such a locus)
            const u32 key = tag | (pr.x + 1u);
            u32 q = home + home_off(pr.x + 1u, H);
            bool found = false;
            for (u32 it = 0; it < (u32)TSLOTS; ++it) {   // (the table always has a free slot)
                const uint2 t = tab_get(*L, q);
                if (t.x == key) { found = t.y == pr.y; break; }
                if (t.x == 0u) break;
                q = next_slot(key, q, it);
            }
            if (!found) return CMP_DIFFERENT;
        }
        return CMP_EQUAL;
    }
};

// VERIFY = false: the hot kernel.  VERIFY = true: the exactness pass (same tiling, compares instead of inserting).
//
// A wave walks its slice in tiles of WT records that start at multiples of WT: every record is loaded exactly once (plus
// the tail a slice's last read hangs into the next slice).  Reads are NOT looked up tile by tile: a *pass* collects the
// {(read, locus) -> mask} entries of up to 1 << lg reads (at most WMAXR) from as many consecutive tiles as fit, and only then
// is every entry hashed and every finished read looked up, one lane each -- a *flush*.  (One flush per tile left three
// quarters of phase (c)'s lanes idle on config 3 -- fifteen reads per tile -- and paid the EC table's round trip, the per-pass
// LDS clear and the hashing loop's ramp four times as often.)  A pass is flushed behind a tile when, going by that tile, the
// next one would bring more records than the table has room for entries or more reads than the pass has room for; a tile whose
// records turn out not to fit after all (every record may make an entry) is held back, still in its registers, until the pass
// has been flushed.  The read that is open at a flush is not read again: its entries so
// far are carried in LDS into the next pass and inserted there with the next tile's records.  A read that would carry more
// than CMAX entries goes to k_slow.  A tile with more reads than the pass has room for (short reads) is worked off in
// several visits: every further visit loads the tile again.
// (RANGES: the reference_start ranges of ECB_F_RANGES updated in the same pass -- more registers, four waves per SIMD)
template <bool VERIFY, bool RANGES = false>
__global__ __launch_bounds__(TPB, RANGES ? (WAVES_PER_SIMD < 4 ? WAVES_PER_SIMD : 4) : WAVES_PER_SIMD) void k_stream(StreamArgs A) {
    __shared__ WaveLds wl[NWAVE];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    WaveLds& L = wl[w];
    // Persistent waves: the launch holds only as many waves as are resident at once, and every wave takes the next
    // unclaimed slice of the stream when it has finished one.  (Slices bound to workgroups at launch left a SIMD slot
    // idle until the slowest of a workgroup's four waves was done, and the last round ragged: a fifth of the kernel.)
    const u64 pw = (u64)blockIdx.x * NWAVE + w;   // this wave
    const StreamCold* const C = A.cold;
    static_assert(WT == 512, "tile index = record index >> 9");
    u32 my_valid = 0, my_new = 0;                 // per lane; a wave sees far fewer than 2^32 records  (records OFFERED, bam_utils.py:261,
                                                  //  are simply the batch's length: the host adds it)
    u32 bad = 0;
    // this wave's current reservation in the key arena: what the last launch left of it is used first (a stream pushed in
    // many small batches would otherwise leave the tail of a 512-pair chunk behind per wave and launch)
    if (lane == 0) L.ws[7] = 0u;
    if (!VERIFY && lane == 0) { const u64* wa = C->wave_arena; const u64 ca = wa[2 * pw]; L.ws[2] = (u32)ca; L.ws[3] = (u32)(ca >> 32); L.ws[4] = (u32)wa[2 * pw + 1]; }
#ifdef ECB_TIMING
    u64 tacc[ECB_TIMING_WORDS] = {}, tlast = __builtin_readcyclecounter();
#endif
    // this wave's per-pass LDS state: table, hash sums, pair counts -- cleared here and behind every flush
    auto clear_pass = [&](u32 ln) {
        uint4* z = tab_base(L);
        u32 zz;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zz));          // (a zero the compiler cannot keep in four registers across the loop)
        const uint4 zv = make_uint4(zz, zz, zz, zz);
#pragma unroll
        for (int t = 0; t < TAB_BYTES / (16 * 64); ++t) z[t * 64 + ln] = zv;
        if constexpr (KS_SHORT) { reinterpret_cast<uint4*>(L.acc)[ln] = zv; reinterpret_cast<u32*>(L.npair)[ln] = zz; }      // (WMAXR = 128 of each)
        else { *reinterpret_cast<uint2*>(&L.acc[ln]) = make_uint2(zz, zz); L.npair[ln] = (unsigned short)zz; }
    };
    clear_pass(lane);                             // (every slice leaves the table as it found it: empty)
    wave_sync();
  for (;;) {
    u32 wid = 0;                                  // the slice (fewer than 2^32 of them: a slice is at least a tile)
    if (lane == 0) wid = (u32)atomicAdd(&A.ctr->next_slice, 1ull);
    wid = (u32)__builtin_amdgcn_readfirstlane((int)wid);
    const u64 chunk = C->chunk;
    const u64 c0 = (u64)wid * chunk;              // (a multiple of WT)
    if (c0 >= A.n) break;
    const u64 c1 = min(c0 + chunk, A.n);
    // resume point: the first record not yet consumed by a finished read (a fresh slice: c0; after a park: the head of the
    // read that was open, or the tile that was next), and how far the slice's records have been counted
    const u64 p = C->resume[2 * (u64)wid], counted0 = C->resume[2 * (u64)wid + 1];
    if (p >= A.n || p == ~0ull) continue;         // finished before a relaunch
    // The loop below thinks in tiles (32-bit indices: scalar registers are scarce): tile t covers records [512 t, 512 t + 512)
    u32 tix = (u32)(p >> 9);                      // the tile to work on
    const u32 c1t = (u32)((c1 + (u64)(WT - 1)) >> 9);             // my slice ends before this tile
    const u32 last_t = (u32)((A.n - 1) >> 9);                     // the stream's last tile ...
    const u32 last_rel = (u32)(A.n - ((u64)last_t << 9));         // ... and how many records it holds
    const u32 counted_t = (u32)((counted0 + (u64)(WT - 1)) >> 9); // tiles before this one have been counted (after a park)
    int p_rel = (int)(p - ((u64)tix << 9));       // (only matters in the first tile after a park)
    // read id of the record before the tile; the first head at or after p starts read prev + 1, and records before it that
    // are not heads belong to the read before (not mine)
    u32 prev = p == 0 ? C->prev_rid : A.rid[rec_at(p - 1, A_TW(A))];
    // The pass: reads pb .. pb + npend - 1 are complete and wait for their lookup, read pb + npend is open (if `open`; the
    // record index of its head: L.ws[0..1]).  Invariant at the start of a tile's first visit: pb + npend + open == prev + 1,
    // the id of the next read to start.
    // The record the slice is taken up at after a park: the head of read pb, or a tile boundary before it -- L.ws[5..6].
    u32 pb = prev + 1u, npend = 0, n_ent = 0;     // n_ent: entries in L.ent (complete reads' and the open read's)
    ws_put64(L, 5, p, lane);
    bool open = false;
    u32 carry_n = 0;                              // entries in L.carry: the open read's, waiting to go into the fresh table
    u32 lgf = pack_lgf(LGMAX);                    // the pass has room for 1 << lg reads, lg = lgf >> 24 (see WaveLds: the table's geometry; pack_lgf)
    bool revisit = false;                         // the tile has been visited before (more reads in it than a pass takes)
    TileRegs R;
    load_tile(A, (u64)tix << 9, min(((u64)tix << 9) + (u64)WT, A.n), lane, R);
    int r_pos[RANGES ? RPL : 1];                  // ECB_F_RANGES: reference_start of the tile's records, prefetched with them
    if constexpr (RANGES) load_pos(A.pos, (u64)tix << 9, min(((u64)tix << 9) + (u64)WT, A.n), lane, r_pos);
    u32 parked = __hip_atomic_load(&A.ctr->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" : "+v"(parked));          // (settled before the loop: otherwise the loop header carries an s_waitcnt vmcnt(0) that every tile pays)
    bool slice_done = false;

    while (!slice_done) {
        // the EC table filled up somewhere: the host grows it and relaunches.  What the pass holds is dropped: the slice is taken up
        // again at the head of the pass's first read (L.ws[5..6]), and looking a read up twice changes nothing.
        if (__builtin_amdgcn_readfirstlane((int)parked)) break;
                                      // (readfirstlane: every lane loaded the same word; said so, the loop is uniform to the compiler --
                                      //  as a per-lane condition it dragged exec-mask bookkeeping through every block of the tile)
        // (opaque per tile: the LDS addresses and constants derived from the lane index are cheap to recompute; hoisted out of
        //  the loop they sat in registers the tile needs, and what did not fit was spilled and re-loaded BEHIND the prefetch)
        u32 ln = lane;
        asm volatile("" : "+v"(ln));
        tix = (u32)__builtin_amdgcn_readfirstlane((int)tix);
        prev = (u32)__builtin_amdgcn_readfirstlane((int)prev);
        pb = (u32)__builtin_amdgcn_readfirstlane((int)pb);
        npend = (u32)__builtin_amdgcn_readfirstlane((int)npend);
        n_ent = (u32)__builtin_amdgcn_readfirstlane((int)n_ent);
        lgf = (u32)__builtin_amdgcn_readfirstlane((int)lgf);
        const u32 lg = lgf >> 24;
        // The table's geometry (see WaveLds): two wave-uniform numbers
        const u32 gp = ((u32)TBASE >> lg) + (TSLOTS == 896 ? (256u >> lg) : 0u) + ((u32)(TBASE / 4) >> lg);
        const HomeGeo HG = home_geo(lgf);
        bool do_flush = false, again = false, more = false;
        bool preflush = false;                     // this tile's records might not fit the pass's table: flush first, then take the tile again
        bool taken = false;                        // the prefetched tile has been waited for (on this path)
        u32 parked_next = parked;
        u32 last_pos = 0xFFFFFFFFu;                // tile-relative head of the tile's last read, if it started here (it may stay open)
        u32 last_rid = prev;
        u32 est = 64;                              // reads a tile brings, going by this one: the next pass's geometry
        const bool ends = tix == last_t;           // batches end on a read boundary
        const bool own = tix < c1t;               // heads in this tile start reads of my slice (tiles do not straddle its end)
        const int te_rel = ends ? (int)last_rel : WT;
        // records offered / valid are counted tile by tile: every tile of my slice once (after a park the tiles before the
        // one that was next have been counted: `counted0` is a tile boundary)
        const bool count_tile = own && tix >= counted_t && !revisit;
        const bool plain = p_rel == 0 && te_rel == WT;      // a whole tile, nothing masked: all but the first after a park / the last of the stream
        // ---- (a) filter, heads -------------------------------------------------------------------
        // Written with integer bit arithmetic throughout: every instruction costs an issue slot, and
        // compare -> mask -> select chains were a third of this kernel's instruction count.
        // Per record: its LDS key (locus + 1 | index of its read within the pass << KBITS) and its haplotype bit -- all that
        // phase (b) needs of it; which records phase (b) takes at all (valid, of a read of this pass) is settled here too:
        // reads are numbered consecutively by the run counter, so "one of the pass's reads" is one unsigned comparison.
        u32 r_key[RPL], r_bit[RPL];
        u32 m_act = 0, m_head = 0;                 // bit k: valid record of a read of this pass / head
        const u32 lim = own ? (1u << lg) : (open ? npend + 1u : 0u);   // (past my slice only the open read is mine)
        // Most tiles lie wholly inside the pass: their first record belongs to a read of the pass (the open one, or the first to start)
        // and their last read still has room -- then every record is "mine" and the per-record test is not made.
        const u32 rid_first = (u32)__builtin_amdgcn_readfirstlane((int)R.rr[0]), rid_last = (u32)__builtin_amdgcn_readlane((int)R.rr[RPL - 1], 63);
        const bool all_mine = rid_first - pb < lim && rid_last - pb < lim && rid_last >= rid_first;
        {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int i0 = g * 256 + 4 * (int)ln;
                // the record before this group's first: the previous ln's last record of the group, or (ln 0) the
                // previous group's very last record
                const u32 up = lane_above(R.rr[4 * g + 3]);
                const u32 wrap = g == 0 ? prev : (u32)__builtin_amdgcn_readlane((int)R.rr[4 * (g > 0 ? g - 1 : 0) + 3], 63);
                u32 in4 = 0xFu, te4 = 0xFu;                                      // records of the tile / at or after p
                if (!plain) {
                    te4 = (1u << clamp04(te_rel - i0, 0, 4)) - 1u;
                    in4 = te4 & ~((1u << clamp04(p_rel - i0, 0, 4)) - 1u);
                }
                const u32 prev0 = ln == 0 ? wrap : up;
                u32 ok4 = 0, head4 = 0, hap_or = 0, mine4 = 0;
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    // record filter (bam_utils.py:264-270): not unmapped, and if paired: read1, proper, mate on the same
                    // reference, next_pos >= 0  <=>  ((f ^ 2) & 0x3082) == 0.  Worked out in the sign bit: x - 1 is negative only
                    // for x = 0, a shift puts a flag bit there, and one funnel shift moves the verdict into the group's mask.
                    const u32 f = R.hh[4 * g + j];
                    const u32 pair_ok = ((f & 0x3082u) ^ 0x2u) - 1u;                              // bit 31
                    const u32 ok31 = ~(f << 29) & (~(f << 31) | pair_ok);                        // bit 31: !unmapped && (!paired || pair_ok)
                    ok4 = __builtin_amdgcn_alignbit(ok4, ok31, 31);                              // ok4 = ok4 << 1 | verdict
                }
                // The rest is per record position, and only for positions at which SOME lane holds a valid record: in a paired-end
                // stream every second record is a mate the filter drops -- wave-uniform branches, two positions each.
#pragma unroll
                for (int par = 0; par < 2; ++par) {
                    if (__ballot((ok4 & (par ? 0xAu : 0x5u)) != 0u) != 0ull) {
#pragma unroll
                        for (int j = par; j < 4; j += 2) {
                            const int k = 4 * g + j;
                            const u32 f = R.hh[k];
                            const u32 step = R.rr[k] - (j == 0 ? prev0 : R.rr[k > 0 ? k - 1 : 0]);
                            const u32 relx = R.rr[k] - pb;                   // (records of reads before the pass's first: huge)
                            const u32 t = R.ll[k] + 1u;
                            r_key[k] = t | (relx << KBITS);
                            r_bit[k] = 1u << ((f >> ECB_HAP_SHIFT) & 31u);
                            // (a haplotype index of 32 or more would alias a low one, a locus of KMASK or more the read tag of the
                            //  LDS keys: both show in the bits from 21 up)
                            hap_or |= ((t & ~KMASK) | f) & (u32)((int)(ok4 << (31 - j)) >> 31);
                            head4 |= (step & 1u) << j;
                            if (!all_mine) mine4 |= (relx < lim ? 1u : 0u) << j;
                        }
                        if constexpr (RANGES) {
                            // reference_start ranges per target (bam_utils.py:282-286), in the pass that has the record in registers anyway:
                            // the 2 x n_loci x n_haps bounds stay in L2, and a record only issues an atomic when it moves a bound (almost
                            // none do after the first few thousand).  Re-running a tile (park, further visits) changes nothing: min / max.
                            if (!revisit) {
                                const u32 nl = C->n_loci, nh = C->n_haps;
                                int2* const rng = A.rng;
                                u32 sl[2]; int2 cur[2]; bool go[2];
#pragma unroll
                                for (int j = par; j < 4; j += 2) {
                                    const int k = 4 * g + j;
                                    const u32 lc = R.ll[k], hap = (R.hh[k] >> ECB_HAP_SHIFT) & 0xFFu;
                                    go[j >> 1] = ((ok4 >> j) & 1u) && lc < nl && hap < nh;       // (out of range: reported at emit)
                                    sl[j >> 1] = lc * nh + hap;
                                    cur[j >> 1] = make_int2(0, 0);
                                    if (go[j >> 1]) cur[j >> 1] = rng[sl[j >> 1]];
                                }
#pragma unroll
                                for (int j = par; j < 4; j += 2) {
                                    const int ps = r_pos[RANGES ? 4 * g + j : 0];
                                    if (go[j >> 1] && ps < cur[j >> 1].x) atomicMin(&rng[sl[j >> 1]].x, ps);
                                    if (go[j >> 1] && ps > cur[j >> 1].y) atomicMax(&rng[sl[j >> 1]].y, ps);
                                }
                            }
                        }
                    } else {
#pragma unroll
                        for (int j = par; j < 4; j += 2) {   // (no lane has a record at these positions: any value will do, none is used)
                            asm volatile("" : "=v"(r_key[4 * g + j])); asm volatile("" : "=v"(r_bit[4 * g + j]));
                        }
                    }
                }
                // the run counter may only step by 0 or 1, and only on a valid record: then, and only then, the steps seen at the
                // valid positions add up to the whole difference
                const u32 big = (u32)(R.rr[4 * g + 3] - prev0 != (u32)__popc(head4));
                if (count_tile) my_valid += __popc(ok4 & te4);
                ok4 &= in4; head4 &= in4;
                bad |= ((p_rel == 0 ? big : 0u) | (head4 & ~ok4)) ? ERR_CONTRACT : 0u;   // (the tile a park resumes in was checked before the park)
                bad |= (hap_or >> (ECB_HAP_SHIFT + (KS_SHORT ? 3 : 5))) ? ERR_RANGE : 0u;      // (indices below 32 -- below 8 where the masks are bytes -- are checked against n_haplotypes per EC, at emit)
                m_act |= (all_mine ? ok4 : (ok4 & mine4)) << (4 * g); m_head |= head4 << (4 * g);
            }
        }
        TICK(0);
        if (__ballot(bad != 0u)) break;            // never index LDS with a broken run counter
        const u32 cnts = wave_sum((u32)__popc(m_head) | ((u32)__popc(m_act) << 16));
        const u32 nheads = cnts & 0xFFFFu, n_mine = cnts >> 16;   // heads; records that go into the pass's table
        last_rid = (u32)__builtin_amdgcn_readlane((int)R.rr[RPL - 1], 63);   // (of a full tile; a short one ends the stream)
        // Reads with records in this tile that are mine: the open one (index npend of the pass) and one per head whose read has not
        // been dealt with on an earlier visit -- heads number their reads prev + 1 ..., the next read to start is pb + npend + open.
        // All but the last are complete here; the last one is too if the stream ends with the tile.  In a tile past my slice only
        // the open read is mine, and it is complete as soon as a head shows up.
        const u32 o1 = open ? 1u : 0u;
        const u32 n_new = own ? (prev + 1u + nheads) - (pb + npend + o1) : 0u;
        const u32 n_in = o1 + n_new;
        est = n_in;
        // Every record may make an entry of its own.  Behind a flush a tile always fits (CMAX carried entries + WT records); a pass that
        // has taken tiles before was judged, after the last of them, to have room for one more like it -- when that turns out wrong
        // (rare), the pass is flushed with the tile untouched in its registers and the tile is then taken again.
        if (n_ent + carry_n + n_mine > (u32)(WT + CMAX)) { preflush = true; do_flush = true; }
        else {
        if (own) {
            if (npend + n_in > (1u << lg)) { again = true; npend = 1u << lg; open = false; }      // (the reads that fit are all complete: more follow)
            else if (n_in) { npend += ends ? n_in : n_in - 1u; open = !ends; }
        } else if (open && (nheads || ends)) { npend += 1u; open = false; }
        more = !ends && (tix + 1u < c1t || open);
        TICK(1);
        // ---- prefetch the next tile while this one is hashed and looked up --------------------------
        // Into the SAME registers: phase (a) has turned the tile into keys and bits, nothing reads R again.  The lane offset of
        // the loads is made to depend on phase (a)'s results, so that the scheduler cannot start them while R is still being read
        // (it did, and a second set of 24 registers plus 24 moves per tile was the price).
        if (more || again) {
            u32 lp = ln;
#pragma unroll
            for (int k = 0; k < RPL; ++k) asm volatile("" : "+v"(lp) : "v"(r_key[k]), "v"(r_bit[k]));
            asm volatile("" : "+v"(lp) : "v"(m_act), "v"(m_head), "v"(bad), "v"(my_valid));
            const u64 nt = (u64)(again ? tix : tix + 1u) << 9;
            load_tile(A, nt, min(nt + (u64)WT, A.n), lp, R);
            if constexpr (RANGES) load_pos(A.pos, nt, min(nt + (u64)WT, A.n), lp, r_pos);
            parked_next = __hip_atomic_load(&A.ctr->full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!again) {                                               // head of the tile's last read (kept if it stays open): the tile's last head
            const u64 h1 = __ballot((m_head >> 4) != 0u), h0 = __ballot((m_head & 15u) != 0u);
            if (h1 | h0) {
                const u32 l = 63u - (u32)__builtin_clzll(h1 ? h1 : h0);
                const u32 bits = (u32)__builtin_amdgcn_readlane((int)m_head, (int)l);
                const u32 k = 31u - (u32)__builtin_clz(h1 ? bits & 0xF0u : bits & 0xFu);
                last_pos = (k & 3u) + (k >> 2) * 256u + 4u * l;
            }
            if (open && last_pos != 0xFFFFFFFFu) ws_put64(L, 0, ((u64)tix << 9) + last_pos, ln);   // (else: the open read stays the open read)
        }

        // ---- (b) the pass's {(read, locus) -> haplotype mask} table in LDS ------------------------------------
        // Staged so that the 8 records' LDS round trips overlap: compare-and-swap on the key, OR of the bit.
        // A ln whose CAS created an entry queues it; every entry is hashed once, at the flush, when all masks are final.
        TICK(2);
        if (!ABL(A, 1u)) {
            // What the open read brought along from the pass before goes in WITH the records, as one more compare-and-swap per lane in the same
            // round (a chain of LDS round trips of its own cost a fifth of the tile): entry c of the carry list is lane c's
            // ninth "record" -- its haplotype "bit" is the whole mask so far.  (More than 64 of them: a second such round.)
            const bool cin = carry_n != 0u;                      // (only right behind a flush: the open read is read 0 of the pass, tag 0)
            u32 q[RPL + 1], old[RPL + 1], act = m_act;
            u32 cb = 0;                                          // my record positions whose first slot is taken by another (read, locus)
            u32 c_key = 0, c_bit = 0;
            if (cin && ln < carry_n) { const uint2 cv = L.carry[ln]; c_key = cv.x; c_bit = cv.y; act |= 1u << RPL; }
            // Two rounds: the even record positions (and the carried entry), then the odd ones -- nine compare-and-swap
            // results in flight at once are more registers than the kernel has, and in a paired-end stream the odd (or the
            // even) positions are the mate records, which the filter drops: a round no lane has a record in is skipped.
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32 hmask = h ? 0x0AAu : 0x155u;           // positions of this round (bit RPL: the carried entry)
                if (__ballot((act & hmask) != 0u) == 0ull) continue;
#pragma unroll
                for (int k = h; k <= RPL; k += 2) {  // (lanes without a record here swap nothing: they expect a value no slot ever holds, at a slot of their own)
                    const u32 key = k < RPL ? r_key[k < RPL ? k : 0] : c_key;
                    q[k] = (act >> k & 1u) ? (key >> KBITS) * gp + home_off(key, HG) : ln;
                }
#pragma unroll
                for (int k = h; k <= RPL; k += 2)
                    old[k] = atomicCAS(tab_key(L, q[k]), (act >> k & 1u) ? 0u : 0xFFFFFFFFu, k < RPL ? r_key[k < RPL ? k : 0] : c_key);
#pragma unroll
                for (int k = h; k <= RPL; k += 2) {
                    const u32 key = k < RPL ? r_key[k < RPL ? k : 0] : c_key, bit = k < RPL ? r_bit[k < RPL ? k : 0] : c_bit;
                    const bool on = act >> k & 1u;
                    const bool made = on && old[k] == 0u;                // this lane created the (read, locus) entry
                    const bool hit = made || (on && old[k] == key);
                    cb |= (on && !hit ? 1u : 0u) << k;
                    tab_or(L, q[k], hit ? bit : 0u);         // duplicate (read, target) records vanish here: bam_utils.py:322-325
                    const u64 mm = __ballot(made);
                    if (made) L.ent[n_ent + __builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u))] =
                        (unsigned short)(KS_SHORT ? q[k] : (q[k] | ((key >> KBITS) << SBITS)));
                    n_ent += (u32)__popcll(mm);
                }
            }
            const bool anyc = cb != 0u;
            if (__ballot(anyc) || (cin && carry_n > 64u)) {
#ifdef ECB_TIMING
                tacc[7] += 1;                                    // (profiling: tiles that take the probe-on path)
#endif
                if (ln == 0) L.ws[7] += 1u;                      // tiles on this path: what the library picks the compilation for the next batch by
                // Probe on -- the records that found their first slot taken, and only they.  They are STAGED -- (key, haplotype bit) appended to the
                // carry list's slots, which are free by now -- and then seated one record per lane, every lane walking its own probe sequence:
                // one copy of the walk for all nine record positions, a round trip per probe whatever the number of records.  (Round 3 walked
                // position by position, lanes idle, starting with the slot just found taken: a third of the kernel on streams with loci anywhere
                // among the targets, `c3r`.  An unrolled round over all positions at once was as fast but doubled the kernel's scalar spills and
                // cost config 2 and the short-read stream 4 - 15 %: profiles/r04_ab_4way.txt.)  Carried entries beyond the 64 that went in as a
                // lane's ninth record are already in the list: they are seated the same way, from their home slot.
                u32 lo_ = 0, hi_ = 0;
                bool from_home = cin && carry_n > 64u;
                if (from_home) { lo_ = 64u; hi_ = carry_n; }
                for (;;) {
                    if (!from_home) {
                        if (!__ballot(cb != 0u)) break;
                        wave_sync();                             // (every lane has read what it needed of the list)
                        u32 n_st = 0;
#pragma unroll
                        for (int k = 0; k <= RPL; ++k) {
                            const bool c = cb >> k & 1u;
                            const u64 mm = __ballot(c);
                            if (!mm) continue;
                            const u32 at = n_st + __builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u));
                            if (c && at < (u32)CMAX) {           // (a list of CMAX: what does not fit waits for the next turn of the loop)
                                const u32 key = k < RPL ? r_key[k < RPL ? k : 0] : c_key, bit = k < RPL ? r_bit[k < RPL ? k : 0] : c_bit;
                                L.carry[at] = make_uint2(key, bit);
                                cb &= ~(1u << k);
                            }
                            n_st = min(n_st + (u32)__popcll(mm), (u32)CMAX);
                        }
                        lo_ = 0u; hi_ = n_st;
                        wave_sync();
                    }
                    for (u32 base = lo_; base < hi_; base += 64u) {
                        const bool have = base + ln < hi_;
                        const uint2 rec = L.carry[have ? base + ln : 0u];
                        bool todo = have, made = false;
                        u32 it = from_home ? 0xFFFFFFFFu : 0u, qq = 0;
                        while (__ballot(todo)) {
                            if (todo) {
                                qq = it == 0xFFFFFFFFu ? (rec.x >> KBITS) * gp + home_off(rec.x, HG) : probe_slot(rec.x, it);
                                const u32 o = atomicCAS(tab_key(L, qq), 0u, rec.x);
                                if (o == 0u || o == rec.x) { todo = false; made = o == 0u; tab_or(L, qq, rec.y); }
                                else if (++it == (u32)TSLOTS) { bad |= ERR_INTERNAL; todo = false; }   // (the table always has a free slot: the bound only keeps
                            }                                                                          //  corrupted state from spinning a wave for ever)
                        }
                        const u64 mm = __ballot(made);
                        if (made) L.ent[n_ent + __builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u))] =
                            (unsigned short)(KS_SHORT ? qq : (qq | ((rec.x >> KBITS) << SBITS)));
                        n_ent += (u32)__popcll(mm);
                    }
                    from_home = false;
                }
            }
            carry_n = 0;
        }
        TICK(3);
        // Flush now?  The stream or my slice ends here; the tile is not done (more reads in it than the pass had room for); or, going
        // by this tile, the next one would bring more records than the table has room for entries, or more reads than the pass has room for.
        do_flush = (npend != 0u || open) &&
                   (!more || again || n_ent + n_mine > (u32)(WT + CMAX) || npend + (open ? 1u : 0u) + n_new > (1u << lg));
        }

        bool giant = false;
        u32 new_carry = 0;
        if (do_flush) {
            wave_sync();
            // every entry is hashed once, now that its mask is final; the entries of a read that stays open are not: they go to
            // the carry list instead (same pass over the queue, no LDS round trips of their own)
            u32 cn = 0;
            const u32 rl_last = npend;                               // the open read's index in the pass: its entries are kept
            const bool keep = open;
            for (u32 e0 = 0; e0 < n_ent; e0 += 64) {
                const u32 e = e0 + ln;
                const bool have = e < n_ent;
                const u32 en = have ? L.ent[e] : 0u, qq = en & SMASK;
                const uint2 en2 = tab_get(L, qq);
                const u32 rl = KS_SHORT ? en2.x >> KBITS : en >> SBITS;      // (128 reads: the queue holds the slot alone, the key says whose entry it is)
                const bool kept = have && keep && rl == rl_last;
                if (have && !kept) {
                    atomicAdd(&L.acc[rl], pair_hash64((en2.x & KMASK) - 1u, en2.y));
                    atomicAdd(reinterpret_cast<u32*>(&L.npair[rl & ~1u]), (rl & 1u) ? 0x10000u : 1u);   // two 16-bit counters per word
                }
                if (keep) {
                    const u64 mm = __ballot(kept);
                    const u32 at = cn + __builtin_amdgcn_mbcnt_hi((u32)(mm >> 32), __builtin_amdgcn_mbcnt_lo((u32)mm, 0u));
                    if (kept && at < (u32)CMAX) L.carry[at] = make_uint2(en2.x & KMASK, en2.y);
                    cn += (u32)__popcll(mm);
                }
            }
            if (keep) { new_carry = cn; giant = cn > (u32)CMAX; }
            wave_sync();

            TICK(4);
            // ---- (c) one ln per read: EC lookup with exact key compare; a new EC gets its key from the pass's LDS table ---------
            // (64 reads at a time: a pass of short reads holds up to 128, and the table they are compared with is the same)
            const u32 nhalf = KS_SHORT ? ((u32)__builtin_amdgcn_readfirstlane((int)npend) + 63u) >> 6 : 1u;
            // (asking for the second 64 reads' table lines before the first 64 are looked up -- one word per lane, waited for in front of the second round --
            //  was measured: 6.16 -> 6.4 ms on the diploid stream, 6.9 with a non-temporal load; not kept)
          for (u32 half = 0; half < nhalf; ++half) {
            u64 j = 0;
            u32 st = ST_NONE, probes = 0, np = 0, fseen = 0;       // fseen: ~(first read) as the slot's line showed it (0 = nothing yet)
            u64 lo = 0;
#ifdef ECB_TIMING
            u32 f_rounds = 0, f_claim = 0;                          // trips to the EC table in this lookup; those in which no lane loaded a line
#endif
            const u32 rx = KS_SHORT ? ln + (half << 6) : ln;       // my read's index within the pass
            const bool on = rx < npend && !ABL(A, 3u);
            const u32 rd = pb + rx;
            LdsSetCmp cmp;
            cmp.L = &L; cmp.cold = C; cmp.home = rx * gp; cmp.H = HG; cmp.tag = rx << KBITS; cmp.np = 0;
            if (on) {
                np = L.npair[rx];
                cmp.np = np;
                lo = finish_hash(L.acc[rx], np);
                j = lo & A.cap_mask;
                if ((u64)rd >= A.reads_hi) bad |= ERR_CONTRACT;          // the run counter ran past what this batch announced
                else st = ST_LOOK;
            }
            if (VERIFY) {                                               // exactness pass: set of this read == key of its EC ?
                if (st == ST_LOOK) {
                    const u32 sl = A.read_slot[rd];
                    bool same = false;
                    if (sl != PENDING) {
                        const uint4* q = reinterpret_cast<const uint4*>(A.table + sl);
                        const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
                        if (a.z != 0u && a.z != DEAD_KEY) {
                            int r = cmp.quick(make_view(a, b, c, d));
                            if (r == CMP_UNSURE) r = cmp.full(A.table + sl, a.z - 1u, a.w);
                            same = r == CMP_EQUAL;
                        }
                    }
                    if (!same) my_new += 1;                             // (counted as "mismatches" in verify mode)
                }
                parked = parked_next; taken = true;
                        } else {
                // Lookup; founders publish their keys; THEN lanes whose slot was claimed but not (visibly) complete settle it --
                // the founder such a ln waits for may be a ln of this very wave.  One round in all but a handful of flushes.
                for (u32 round = 0;; ++round) {
                    if (st == ST_LOOK) {
                        if (ABL(A, 64u)) { st = ST_HIT; fseen = 0xFFFFFFFFu; }   // (profiling: no table access at all, no first-read atomic)
                        else if (ABL(A, 4u)) st = ST_HIT;
                    }
                    // The lookup in explicit trips to the table: in every trip EVERY unsettled lane has its memory operation in flight -- the four
                    // 16-byte loads of the line it looks at (ST_LOOK) or the compare-and-swap on the slot it found empty (ST_CLAIM) -- and the wave
                    // waits once for the lot.  (table_lookup, one lane's loop run by 64 in lock-step, waited for the first slots' lines, then for the
                    // claims of the lanes that found theirs empty -- the other lanes idle --, and only then sent the lanes whose slot held another
                    // key on to the next: the longest probe sequence among 64 lanes plus one trip per flush, 3.0 on config 3, where two or three
                    // lanes decide the last two of them.  Claims and onward probes now travel together: 2.4.  profiles/flush_rounds_c3.txt)  What a line or a claim's answer means is
                    // table_lookup's reading of it, word for word.
                    for (bool first = round == 0u && half == 0u;; first = false) {
                        const bool look = st == ST_LOOK, claim = st == ST_CLAIM;
#ifdef ECB_TIMING
                        if (__ballot(look || claim)) { f_rounds += 1u; if (!__ballot(look)) f_claim += 1u; }
#endif
                        Slot* const s = A.table + j;
                        // (the loads are not under a branch: the lanes that look at nothing load the table's first line, one request for the lot, and ignore it.
                        //  Loads of the looking lanes alone, merged with zeros for the others, were register copies in the block of the loads -- and a wait
                        //  for every line in front of them, before the claims were issued.)
                        const uint4* const q = reinterpret_cast<const uint4*>(look ? s : A.table);
                        uint4 a = q[0], b = a, c = a, d = a;                  // lo, n1, off | count, first_inv, pair 0 | pairs 1, 2 | pairs 3, 4
                        if (!ABL(A, 16u)) { b = q[1]; c = q[2]; d = q[3]; }  // (profiling only: 16 = first 16 bytes only, 8 = no key compare)
                        u64 got = 0;
                        if (claim) got = atomicCAS(&s->lo, 0ull, lo);
                        // The loads and the compare-and-swap are issued back to back under their execution masks, and the answers are opaque up to
                        // here: left alone, the compiler sinks the compare's first steps into the block of the loads and waits for the lines there,
                        // in front of the claims.
                        asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
                        asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(c.z), "+v"(c.w), "+v"(d.x), "+v"(d.y), "+v"(d.z), "+v"(d.w), "+v"(got));
                        bool adv = false;                                   // on to the next slot
                        if (look) {
                            fseen = 0u;
                            const u64 clo = ((u64)a.y << 32) | a.x;
                            if (clo == 0ull) st = ST_CLAIM;                  // empty as far as this (possibly old) copy of the line shows: the claim tells
                            else if (clo != lo) adv = true;
                            else if (a.z == 0u) st = ST_PENDING;             // claimed with our hash, its key not (visibly) complete
                            else if (a.z == DEAD_KEY) adv = true;
                            else {
                                fseen = b.y;                                 // (what this line -- possibly an old copy -- shows of the EC's first read)
                                if (ABL(A, 8u)) st = ST_HIT;
                                else {
                                    const int r = cmp.quick(make_view(a, b, c, d));
                                    if (r == CMP_EQUAL) st = ST_HIT;
                                    else if (r == CMP_DIFFERENT) adv = true;     // (same hash, another key: a true collision takes the next slot)
                                    else st = ST_PENDING;
                                }
                            }
                        } else if (claim) {
                            if (got == 0ull) st = ST_CREATED;
                            else if (got == lo) st = ST_PENDING;             // claimed with our hash a moment ago: its key decides
                            else adv = true;
                        }
#ifdef ECB_TIMING
                        // (profiling: what the claims of this trip lost to -- a slot taken since its line was read, by another hash or by a founder with mine)
                        tacc[15] += (u64)__popcll(__ballot(claim && got != 0ull && got != lo)); tacc[16] += (u64)__popcll(__ballot(claim && got == lo));
#endif
                        if (adv) { j = (j + 1) & A.cap_mask; ++probes; st = probes < MAX_PROBE ? ST_LOOK : ST_FULL; }
                        if (first) {
                            TICK(5);
                            // Take over the prefetched tile HERE, right behind the lookup's own wait and before this flush issues any store.
                            // vmcnt counts in order: wherever the compiler first touches these registers it waits for everything issued before
                            // that point, and at the end of the tile (where the moves sink to if left alone) or at the top of the next one
                            // (the parked flag) that meant sitting out the round trips of the founders' stores -- ~3000 clocks per tile on C3.
                            parked = parked_next; taken = true;
                        #pragma unroll
                            for (int k = 0; k < RPL; ++k) {
                                asm volatile("" : "+v"(R.rr[k])); asm volatile("" : "+v"(R.ll[k])); asm volatile("" : "+v"(R.hh[k]));
                                if constexpr (RANGES) asm volatile("" : "+v"(r_pos[k]));
                            }
                            asm volatile("" : "+v"(parked));
                        }
                        if (!__ballot(st == ST_LOOK || st == ST_CLAIM)) break;
                    }
                    const u64 cmask = __ballot(st == ST_CREATED);
                    if (cmask) {
                        const bool cr = st == ST_CREATED;
                        const u32 want = cr && np > INL ? np - INL : 0u;    // pairs beyond the slot's own go to the key arena
                        u32 off = 0;
                        if (__ballot(want != 0u)) {
                            const u32 incl = wave_incl_scan(want);
                            const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                            u64 chunk_at = ws_get64(L, 2);
                            u32 chunk_left = (u32)__builtin_amdgcn_readfirstlane((int)L.ws[4]);
                            if (total > chunk_left) {                       // reserve another stretch of the key arena
                                const u32 take = max(total, ARENA_CHUNK);
                                u64 at = 0;
                                if (ln == 0) at = arena_alloc(A.ctr, C->arena_cap, take, (u32)pw);
                                chunk_at = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(at >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)at);
                                chunk_left = take;
                                if (chunk_at == ~0ull) { bad |= ERR_ARENA; chunk_left = 0; }
                            }
                            if (!(bad & ERR_ARENA)) {
                                off = (u32)(chunk_at + (incl - want));       // the arena holds < 2^32 pairs (Slot::off)
                                chunk_at += total; chunk_left -= total;
                            }
                            ws_put64(L, 2, chunk_at, ln);
                            if (ln == 0) L.ws[4] = chunk_left;
                        }
                        const bool dead = (bad & ERR_ARENA) != 0u;           // no room for a long key: the run fails; the slots are marked, not left claimed
                        // The keys are copied by the whole wave from the pass's entry queue (every (read, locus) entry once, any
                        // order: rows are sorted when they are emitted), not by the founding ln walking its read's table:
                        // that serial walk with 1-3 lanes alive was ~400 issue slots per tile, a quarter of the kernel.
                        const u32 j32 = (u32)j;
                        uint2* const arena = C->arena;
                        if (!dead) for (u32 e0 = 0; e0 < n_ent; e0 += 64) {
                            const u32 e = e0 + ln;
                            const u32 en = e < n_ent ? L.ent[e] : 0u, qq = en & SMASK;
                            const u32 rl = KS_SHORT ? tab_get(L, qq).x >> KBITS : en >> SBITS;
                            const u32 o = __shfl(off, rl & 63u), jj = __shfl(j32, rl & 63u);            // (all lanes: the loop bound is uniform)
                            if (e < n_ent && (!KS_SHORT || (rl >> 6) == half) && (cmask >> (rl & 63u) & 1ull) && !ABL(A, 32u)) {    // (32: profiling, no key stores)
                                const u32 was = atomicSub(reinterpret_cast<u32*>(&L.npair[rl & ~1u]), (rl & 1u) ? 0x10000u : 1u);
                                const u32 pos = ((rl & 1u) ? was >> 16 : was & 0xFFFFu) - 1u;   // a place of its own among the read's pairs
                                uint2* dst = pos < INL ? &A.table[jj].pair[pos] : arena + ((u64)o + (pos - INL));
                                const uint2 en2 = tab_get(L, qq);
                                store_wt64(reinterpret_cast<u64*>(dst), pack2(make_uint2((en2.x & KMASK) - 1u, en2.y)));
                            }
                        }
                        if (cr) { publish_key(A.table + j, dead ? DEAD_KEY : np + 1u, off); st = ST_HIT; }   // (no wait: readers tell a whole key from its masks)
                        my_new += (u32)__popcll(cmask);
                    }
                    if (!__ballot(st == ST_PENDING)) break;
                    if (round >= 64u) { if (st == ST_PENDING) { bad |= ERR_INTERNAL; st = ST_NONE; } break; }
#ifdef ECB_TIMING
                    f_rounds += 1u;                                      // (a settle polls the slot: a trip at the least)
                    tacc[17] += (u64)__popcll(__ballot(st == ST_PENDING));   // (profiling: lanes that go through table_settle ...)
                    bool s_other = false;
#endif
                    if (st == ST_PENDING) {
                        const int r = table_settle(A.table + j, cmp);
#ifdef ECB_TIMING
                        s_other = r == ST_OTHER;
#endif
                        if (r == ST_HIT) st = ST_HIT;
                        else if (r == ST_STUCK) { bad |= ERR_INTERNAL; st = ST_NONE; atomicExch(&A.ctr->full, 1u); }   // (every wave stops at its next tile)
                        else { j = (j + 1) & A.cap_mask; ++probes; st = probes < MAX_PROBE ? ST_LOOK : ST_FULL; }
                    }
#ifdef ECB_TIMING
                    tacc[18] += (u64)__popcll(__ballot(s_other));            // (... and those it sent on to the next slot: the slot holds the other key of their hash)
#endif
                }
#ifdef ECB_TIMING
                // trips to the EC table this lookup of up to 64 reads made: a histogram (1, 2, 3, 4 or more), their sum, the claim-only ones, lookups
                tacc[8] += f_rounds <= 1u; tacc[9] += f_rounds == 2u; tacc[10] += f_rounds == 3u; tacc[11] += f_rounds >= 4u; tacc[12] += f_rounds; tacc[13] += f_claim; tacc[14] += 1;
#endif
                if (st == ST_FULL) {                                    // table too full here: defer the read, park
                    atomicExch(&A.ctr->full, 1u);
                    // (its head: the first record of the read among those of my slice up to the tile in hand -- the run counter never decreases)
                    queue_defer(A.ctr, C, tile_head(A.rid, (u64)wid * C->chunk, min(((u64)tix << 9) + (u64)WT, A.n), rd, A_TW(A)));
                } else if (st == ST_HIT) {
                    A.read_slot[rd] = (u32)j;
                    // First appearance of the EC (bam_utils.py:682-698: rank = first-seen order), kept current here: an old copy
                    // of the line can only show a LATER first read, so the comparison errs on the side of one more atomic.
                    if (~rd > fseen) atomicMax(&A.table[j].first_inv, ~rd);
                }
            }
          }
            wave_sync();
            // the next pass: an empty table, its read 0 the read after the ones just looked up (the open one, if there is one)
            clear_pass(ln);
            pb += npend; npend = 0; n_ent = 0;
            const u32 e4 = min(est * (u32)ECB_EST_MUL, 1u << LGMAX);
            lgf = pack_lgf(e4 > 1u ? 32u - (u32)__builtin_clz(e4 - 1u) : 0u);    // room for four tiles like this one, 64 reads at most
            if (open) {
                if (!giant) carry_n = new_carry;
                else {                                               // more entries than a pass carries over: one workgroup for this read (k_slow)
                    if (ln == 0) {
                        queue_defer(A.ctr, C, ws_get64(L, 0));
                    }
                    open = false; pb += 1u;                           // (the rest of a giant read is skipped: not a head, not open, not mine)
                }
            }
            ws_put64(L, 5, open ? ws_get64(L, 0) : (u64)((preflush || again) ? tix : tix + 1u) << 9, ln);
            wave_sync();
            TICK(6);
        }
        if (preflush) { revisit = true; continue; }                  // (the tile is still in its registers: nothing was prefetched over it)
        if (!taken) {                                                // no flush behind this tile: the prefetched one is waited for here
            parked = parked_next;
        #pragma unroll
            for (int k = 0; k < RPL; ++k) {
                asm volatile("" : "+v"(R.rr[k])); asm volatile("" : "+v"(R.ll[k])); asm volatile("" : "+v"(R.hh[k]));
                if constexpr (RANGES) asm volatile("" : "+v"(r_pos[k]));
            }
            asm volatile("" : "+v"(parked));
        }
        if (again) { revisit = true; continue; }                     // same tile, the reads after the ones just looked up (p_rel stays: the tile is loaded again)
        revisit = false; p_rel = 0;
        prev = last_rid;
        slice_done = !more;
        tix += 1u;
    }
    // where a relaunch takes this slice up: at the head of the first read that has not been looked up
    u64 p_out = ws_get64(L, 5);
    const u64 counted = max(counted0, min((u64)(revisit ? tix + 1u : tix) << 9, c1));   // (every tile before tix has been counted; tix itself once its first visit is through)
    const bool stopped = __ballot(bad != 0u) || __builtin_amdgcn_readfirstlane((int)parked);
    if (__ballot(bad != 0u)) { if (bad) atomicOr(&A.ctr->err, bad); p_out = ~0ull; }
    else if (slice_done) p_out = ~0ull;
    if (lane == 0) { u64* rs = C->resume; rs[2 * (u64)wid] = p_out; rs[2 * (u64)wid + 1] = counted; }
    if (stopped) break;
  }
    // records offered / valid: one atomic pair per wave
    const u32 wa = (u32)__builtin_amdgcn_readfirstlane((int)L.ws[7]), wv = wave_sum(my_valid);      // (wa: tile visits on the probe-on path)
    // per-wave totals go to their own words: thousands of waves adding to three shared counters serialise (~50 ns each)
    const u32 wn = VERIFY ? wave_sum(my_new) : my_new;
#ifdef ECB_TIMING
    if (lane == 0 && C->timing) for (int i = 0; i < ECB_TIMING_WORDS; ++i) atomicAdd(C->timing + i, tacc[i]);
#endif
    if (lane == 0) { u32* wc = C->wave_counts; wc[3 * pw] = wa; wc[3 * pw + 1] = wv; wc[3 * pw + 2] = wn; }
    if (!VERIFY && lane == 0) { u64* wav = C->wave_arena; wav[2 * pw] = ((u64)L.ws[3] << 32) | L.ws[2]; wav[2 * pw + 1] = L.ws[4]; }
}
