// ---- --collapse-umis: the reads of one molecule made one read (ecb_collapse_umis / ecb_collapse_umis_device; included by ecb.hip; of
// its siblings it needs none: Call, the lowest-offender word, tuple_step, Arena and the span check are ecb.hip's) -----------------------
// The rule is include/ecb_umi.h's -- bus2ec's, stated on tuple streams.  Every step is a map over an array (one element per thread:
// UMI_LANE_RECS = 1, a wave UMI_WAVE_RECS = 64, a workgroup UMI_WG_RECS = TPB, whatever n is), one of the library's scans (scan_launch)
// or its stable LSD sort (radix_sort_pairs64); every place written is computed from scans, nothing is placed by an atomic, so every output
// is a function of the input alone.  The only atomic is the atomicMin of the lowest offender (offender, ecb.hip), which only a refusal reads.
// A run of any length -- a molecule of every read -- is measured by two scan values, never walked: there is no "long run" path.
//   1. k_umi_check: 12 bytes per record in.  The contract against the record before, locus and haplotype of a passing record, the
//      filter's verdict per record (pass), whether the first id has a passing record.  || read back: refusals, the number of reads.
//      From here on a read's index is read_id - base: validated.  scan(pass) -> ppos.  k_umi_reads: where every read starts.
//   2. (mol_key, read) sorted on all 64 bits; k_umi_heads: a run of equal keys starts a molecule, every ECB_UMI_NONE read one of its own;
//      scan.  k_umi_mols: a molecule's place in the sorted order, whether a read is its molecule's first (the sort is stable: the lowest
//      index), whether it has k > 1 reads; scan -> the rank mm among those.  k_umi_assign: a read's mm (UMI_NONE: a singleton), a k > 1
//      molecule's first read and k.  || read back.  No k > 1 molecule: steps 3 and 4 are skipped -- singletons never meet the second sort.
//   3. k_umi_mark + scan + k_umi_pairs: the passing records of k > 1 molecules, compacted, as (mm | locus | haplotype, read), each part in the bits its range needs (UmiKey).
//      Sorted on the bits in use: stable, and the stream has the reads ascending, so within a run of equal keys a read's duplicates lie
//      side by side.  k_umi_runs: heads of the (molecule, target) runs and of the distinct reads within them; two scans.
//      k_umi_runstart: the runs listed, and every molecule's first run.
//   4. k_umi_keep: a run's distinct reads = the difference of two scan values; kept iff that is k.  scan -> a kept pair's place.
//   5. k_umi_counts: per first read the records its molecule gives (a singleton its passing records, a k > 1 molecule its kept pairs);
//      scans in read order -> the new ids and the output offsets.  || read back: every size is known, every buffer taken.
//      k_umi_emit_single / k_umi_emit_multi / k_umi_first: the first writes to the caller's memory.
namespace {
constexpr u32 UMI_LANE_RECS = 1;                              // records per lane: every kernel is a map, one element per thread
constexpr u32 UMI_WAVE_RECS = 64 * UMI_LANE_RECS;             // records per wave
constexpr u32 UMI_WG_RECS = (TPB / 64) * UMI_WAVE_RECS;       // records per workgroup
constexpr u32 UMI_HAP_BITS = 5;                               // the second sort's key is mm | locus | haplotype, each in the bits its range needs (UmiKey):
constexpr u32 UMI_LOC_BITS = 26;                              // at the most 30 + 26 + 5 of them
constexpr u32 UMI_MM_BITS = 30;
constexpr u32 UMI_NONE = 0xFFFFFFFFu;                         // a read's mm: its molecule has no other read
constexpr u64 UMI_KEY_NONE = ECB_UMI_NONE;
enum : u32 { UMI_R_LOCUS = TUPLE_R_FILTERED + 1, UMI_R_HAP };      // (the tuple contract's reasons come first: tuple_reason)
static_assert(UMI_R_LOCUS == 4 && UMI_R_HAP == 5, "the reason codes of a refusal do not move");
static_assert(UMI_WG_RECS == (u32)TPB, "a launch of nblk(n, UMI_WG_RECS) workgroups of TPB threads is one element per thread");
static_assert(MAX_LOCI <= 1u << UMI_LOC_BITS && UMI_MM_BITS + UMI_LOC_BITS + UMI_HAP_BITS <= 64, "a molecule's rank, a locus and a haplotype below 32 fit the key");
// where the three parts of the key lie: fewer bits are fewer passes of the sort (config 4's 80 000 loci x 8 haplotypes: 20 bits below the rank, not 31)
struct UmiKey {
    u32 loc_shift, mm_shift, loc_mask;
    static u32 width(u32 top) { return top ? 32u - (u32)__builtin_clz(top) : 0u; }      // bits that hold 0 .. top
    UmiKey(u32 n_loci, u32 n_haps) : loc_shift(width(n_haps - 1)), mm_shift(loc_shift + width(n_loci - 1)), loc_mask((1u << width(n_loci - 1)) - 1u) {}
    u64 bits(u32 n_multi) const { return msb_mask((u64)(n_multi - 1) << mm_shift | ((1ull << mm_shift) - 1ull)); }
};

const char* umi_reason(u32 r) {
    switch (r) {
    case UMI_R_LOCUS: return "locus at or beyond n_loci";
    case UMI_R_HAP: return "haplotype at or beyond n_haps";
    default: return tuple_reason(r);
    }
}
// record i against the record before and against the targets; pass[i]; info[0] = 1 where a passing record carries the first id (that id is
// then read 0, otherwise the records that carry it belong to no read); info[1] = first id | last id << 32
__global__ __launch_bounds__(TPB) void k_umi_check(const u32* rid, const u32* loc, const u32* hf, u64 n, u32 n_loci, u32 n_haps, u64* err, u64* info, u32* pass) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u32 id = rid[i], f = hf[i];
    const bool ok = rec_valid(f);
    if (const u32 why = tuple_step(i ? rid[i - 1] : id, id, ok)) offender(err, i, why);
    if (ok) {
        if (loc[i] >= n_loci) offender(err, i, UMI_R_LOCUS);
        else if ((f >> ECB_HAP_SHIFT) >= n_haps) offender(err, i, UMI_R_HAP);
        if (id == rid[0]) info[0] = 1ull;                     // (every writer stores the same word)
    }
    pass[i] = ok;
    if (i == 0) info[1] = (u64)rid[n - 1] << 32 | id;
}
// the lowest record whose id is `steps` or more above the first (the ids ascend: checked)
__global__ void k_umi_find(const u32* rid, u64 n, u32 steps, u64* out) {
    if (blockIdx.x || threadIdx.x) return;
    u64 lo = 0, hi = n;
    const u32 id0 = rid[0];
    while (lo < hi) { const u64 m = (lo + hi) >> 1; if (rid[m] - id0 < steps) lo = m + 1; else hi = m; }
    *out = lo;
}
// where read r starts (rstart[n_reads] = n); the records in front that carry base - 1 belong to no read
__global__ __launch_bounds__(TPB) void k_umi_reads(const u32* rid, u64 n, u32 base, u32 n_reads, u32* rstart) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    if (i == 0) rstart[n_reads] = (u32)n;
    const u32 r = rid[i] - base;
    if (r < n_reads && (i == 0 || rid[i - 1] != rid[i])) rstart[r] = (u32)i;
}
__global__ __launch_bounds__(TPB) void k_umi_keys(const u64* mol_key, u32 n_reads, u64* keys, u32* vals) {
    const u64 r = blockIdx.x * (u64)TPB + threadIdx.x;
    if (r < n_reads) { keys[r] = mol_key[r]; vals[r] = (u32)r; }
}
__global__ __launch_bounds__(TPB) void k_umi_heads(const u64* keys, u32 n_reads, u32* head) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j < n_reads) head[j] = j == 0 || keys[j] != keys[j - 1] || keys[j] == UMI_KEY_NONE;
}
// sorted place j: whether its read is its molecule's first; at a head, where the molecule starts and whether it has a second read
__global__ __launch_bounds__(TPB) void k_umi_mols(const u64* keys, const u32* vals, const u32* head, const u32* hpos, u32 n_reads, u32 n_mols, u32* isfirst,
                                                  u32* mstart, u32* multi, u64* n_none) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n_reads) return;
    if (j == 0) { mstart[n_mols] = n_reads; *n_none = n_reads - lower_bound_u64(keys, n_reads, UMI_KEY_NONE); }
    isfirst[vals[j]] = head[j];
    if (head[j]) { mstart[hpos[j]] = (u32)j; multi[hpos[j]] = j + 1 < n_reads && !head[j + 1]; }
}
__global__ __launch_bounds__(TPB) void k_umi_assign(const u32* vals, const u32* head, const u32* hpos, const u32* mstart, const u32* multi, const u32* mmpos,
                                                    u32 n_reads, u32* rmm, u32* mm_first, u32* mm_size) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n_reads) return;
    const u32 m = hpos[j] + head[j] - 1u, mm = multi[m] ? mmpos[m] : UMI_NONE;      // (hpos: heads before j)
    rmm[vals[j]] = mm;
    if (head[j] && mm != UMI_NONE) { mm_first[mm] = vals[j]; mm_size[mm] = mstart[m + 1] - mstart[m]; }
}
// the passing records of k > 1 molecules (a record that passes lies in a read: its id stepped on a passing record)
__global__ __launch_bounds__(TPB) void k_umi_mark(const u32* rid, const u32* pass, const u32* rmm, u32 base, u64 n, u32* mark) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) mark[i] = pass[i] && rmm[rid[i] - base] != UMI_NONE;
}
__global__ __launch_bounds__(TPB) void k_umi_pairs(const u32* rid, const u32* loc, const u32* hf, const u32* mark, const u32* cpos, const u32* rmm, u32 base, u64 n,
                                                   UmiKey kf, u64* keys, u32* vals) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n || !mark[i]) return;
    const u32 r = rid[i] - base;
    keys[cpos[i]] = (u64)rmm[r] << kf.mm_shift | (u64)loc[i] << kf.loc_shift | (hf[i] >> ECB_HAP_SHIFT);
    vals[cpos[i]] = r;
}
// sorted by (molecule, target), the reads ascending within: heads of the runs, and of the distinct reads within a run
__global__ __launch_bounds__(TPB) void k_umi_runs(const u64* keys, const u32* vals, u64 m, u32* rhead, u32* dhead) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= m) return;
    const bool h = j == 0 || keys[j] != keys[j - 1];
    rhead[j] = h;
    dhead[j] = h || vals[j] != vals[j - 1];
}
__global__ __launch_bounds__(TPB) void k_umi_runstart(const u64* keys, const u32* rhead, const u32* rpos, u64 m, u32 n_runs, u32 n_multi, UmiKey kf, u32* runstart, u32* mrun) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= m) return;
    if (j == 0) { runstart[n_runs] = (u32)m; mrun[n_multi] = n_runs; }
    if (!rhead[j]) return;
    runstart[rpos[j]] = (u32)j;
    const u32 mm = (u32)(keys[j] >> kf.mm_shift);
    if (j == 0 || (u32)(keys[j - 1] >> kf.mm_shift) != mm) mrun[mm] = rpos[j];
}
// run t is kept iff as many distinct reads name it as the molecule has
__global__ __launch_bounds__(TPB) void k_umi_keep(const u64* keys, const u32* runstart, const u32* dpos, const u32* mm_size, u32 n_runs, UmiKey kf, u32* keep) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t >= n_runs) return;
    const u32 a = runstart[t];
    keep[t] = dpos[runstart[t + 1]] - dpos[a] == mm_size[(u32)(keys[a] >> kf.mm_shift)];
}
// read r: the records its molecule gives out, if r is the molecule's first read (mrun, kpos: null where no molecule has k > 1)
__global__ __launch_bounds__(TPB) void k_umi_counts(const u32* isfirst, const u32* rmm, const u32* rstart, const u32* ppos, const u32* mrun, const u32* kpos,
                                                    u32 n_reads, u32* ocnt, u32* surv) {
    const u64 r = blockIdx.x * (u64)TPB + threadIdx.x;
    if (r >= n_reads) return;
    u32 c = 0;
    if (isfirst[r]) { const u32 mm = rmm[r]; c = mm == UMI_NONE ? ppos[rstart[r + 1]] - ppos[rstart[r]] : kpos[mrun[mm + 1]] - kpos[mrun[mm]]; }
    ocnt[r] = c; surv[r] = c != 0u;
}
// a singleton's passing records as they are, in stream order
__global__ __launch_bounds__(TPB) void k_umi_emit_single(const u32* rid, const u32* loc, const u32* hf, const u32* pass, const u32* ppos, const u32* rstart,
                                                         const u32* rmm, const u32* newid, const u32* ooff, u32 base, u64 n, u32* orid, u32* oloc, u32* ohf) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n || !pass[i]) return;
    const u32 r = rid[i] - base;
    if (rmm[r] != UMI_NONE) return;
    const u32 o = ooff[r] + (ppos[i] - ppos[rstart[r]]);
    orid[o] = newid[r]; oloc[o] = loc[i]; ohf[o] = hf[i];
}
// a k > 1 molecule's kept pairs: the sort left them ascending in (locus, haplotype)
__global__ __launch_bounds__(TPB) void k_umi_emit_multi(const u64* keys, const u32* runstart, const u32* keep, const u32* kpos, const u32* mrun, const u32* mm_first,
                                                        const u32* newid, const u32* ooff, u32 n_runs, UmiKey kf, u32* orid, u32* oloc, u32* ohf) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t >= n_runs || !keep[t]) return;
    const u64 k = keys[runstart[t]];
    const u32 mm = (u32)(k >> kf.mm_shift), f = mm_first[mm], o = ooff[f] + (kpos[t] - kpos[mrun[mm]]);
    orid[o] = newid[f];
    oloc[o] = (u32)(k >> kf.loc_shift) & kf.loc_mask;
    ohf[o] = ((u32)k & ((1u << kf.loc_shift) - 1u)) << ECB_HAP_SHIFT;
}
__global__ __launch_bounds__(TPB) void k_umi_first(const u32* surv, const u32* newid, u32 n_reads, u32* first_read) {
    const u64 r = blockIdx.x * (u64)TPB + threadIdx.x;
    if (r < n_reads && surv[r]) first_read[newid[r]] = (u32)r;
}

int umi_check_args(const void* read_id, const void* locus, const void* hapflag, const void* mol_key, uint64_t n, uint64_t n_reads, uint32_t n_loci, uint32_t n_haps,
                   const void* out_read_id, const void* out_locus, const void* out_hapflag, const void* out_first_read, const void* out_counts) {
    if (!read_id || !locus || !hapflag || !mol_key || !out_read_id || !out_locus || !out_hapflag || !out_first_read || !out_counts || !n)
        return fail(nullptr, ECB_ERR_ARG, "umi: bad argument");
    if (!n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "umi: n_haps out of range (1 .. 31)");
    if (!n_loci || n_loci >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "umi: n_loci out of range (1 .. 2^26-3)");
    if (n >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "umi: 2^30 records or more");                   // (radix_sort_pairs64)
    // (a stream that holds other than n_reads reads is refused later; until then no byte of mol_key or out_first_read beyond n entries counts)
    const u64 nr = std::min<u64>(n_reads, n);
    const std::vector<Span> spans = {{read_id, n * 4}, {locus, n * 4}, {hapflag, n * 4}, {mol_key, nr * 8}, {out_read_id, n * 4}, {out_locus, n * 4},
                                     {out_hapflag, n * 4}, {out_first_read, nr * 4}};
    for (size_t j = 0; j < spans.size(); ++j) if ((uintptr_t)spans[j].p & (j == 3 ? 7u : 3u)) return fail(nullptr, ECB_ERR_ARG, "umi: a pointer that is not aligned to its element");
    if (span_clash(spans, 4)) return fail(nullptr, ECB_ERR_ARG, "umi: an output overlaps an input or another output");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_collapse_umis_device(int device, const void* d_read_id, const void* d_locus, const void* d_hapflag, const void* d_mol_key, uint64_t n,
                                        uint64_t n_reads, uint32_t n_loci, uint32_t n_haps, void* d_out_read_id, void* d_out_locus, void* d_out_hapflag,
                                        void* d_out_first_read, uint64_t* out_counts) {
    RCCHK(umi_check_args(d_read_id, d_locus, d_hapflag, d_mol_key, n, n_reads, n_loci, n_haps, d_out_read_id, d_out_locus, d_out_hapflag, d_out_first_read, out_counts));
    Call c(device, "umi: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u32 *rid = (const u32*)d_read_id, *loc = (const u32*)d_locus, *hf = (const u32*)d_hapflag;
    u32 *orid = (u32*)d_out_read_id, *oloc = (u32*)d_out_locus, *ohf = (u32*)d_out_hapflag;
    // [0] lowest (record << 8 | reason)  [1] the first id has a passing record  [2] first id | last id << 32  [3] the sort's word
    // [4] the record a read starts at  [5] ECB_UMI_NONE reads  [6 ..) scan totals
    u64* words;
    RCCHK(c.status_words(words, 16, 1));
    // the sorts' buffers are the device's pool's; what outlives a sort is cut from one more pool buffer, sized from n alone (a stream holds
    // at most n reads, at most n / 2 molecules of several): eight arrays per record, twelve per read, three per k > 1 molecule, one scan's scratch
    Arena ar(c, CV_X0, 20 * Arena::pad(n + 1, 4) + 3 * Arena::pad(n / 2 + 2, 4) + Arena::pad(scan_words(n + 1), 4));
    u64 *k0 = c.get<u64>(CV_KEYS0, n), *k1 = c.get<u64>(CV_KEYS1, n);
    u32 *v0 = c.get<u32>(CV_VALS0, n), *v1 = c.get<u32>(CV_VALS1, n);
    const SortScratch ss{c.get<u32>(CV_HIST, rs_words(n)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 3};
    RCCHK(c.missing());
    u32 *pass = ar.take<u32>(n), *ppos = ar.take<u32>(n + 1), *sums = ar.take<u32>(scan_words(n + 1));
    RCCHK(ar.missing(c));
    u64 back[16];
    const unsigned grid_n = nblk(n, UMI_WG_RECS);
    // 1. the contract, the reads
    k_umi_check<<<grid_n, TPB, 0, st>>>(rid, loc, hf, n, n_loci, n_haps, words, words + 1, pass);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words, 3));
    RCCHK(refuse_offender(back[0], "umi: record", umi_reason));
    const u32 id0 = (u32)back[2], id_last = (u32)(back[2] >> 32), lead = back[1] ? 0u : 1u;      // (lead: the first id is no read's)
    const u64 in_stream = (u64)(id_last - id0) + 1 - lead;
    if (in_stream != n_reads) {
        u64 at = n - 1;
        if (in_stream > n_reads) {
            k_umi_find<<<1, 64, 0, st>>>(rid, n, (u32)n_reads + lead, words + 4);
            CALLCHK(c, hipGetLastError());
            RCCHK(c.read_back(back, words, 5));
            at = back[4];
        }
        return fail(nullptr, ECB_ERR_CONTRACT, "umi: record %llu: the stream holds %llu reads, n_reads is %llu", (unsigned long long)at,
                    (unsigned long long)in_stream, (unsigned long long)n_reads);
    }
    u64 counts[6] = {n_reads, 0, 0, 0, 0, 0};
    if (!n_reads) { memcpy(out_counts, counts, sizeof counts); return ECB_OK; }      // (no record passes: nothing comes out)
    const u32 R = (u32)n_reads, base = id0 + lead;
    const unsigned grid_r = nblk(R, UMI_WG_RECS);
    u32 *rstart = ar.take<u32>(R + 1), *head = ar.take<u32>(R), *hpos = ar.take<u32>(R + 1), *isfirst = ar.take<u32>(R), *rmm = ar.take<u32>(R);
    u32 *mstart = ar.take<u32>(R + 1), *multi = ar.take<u32>(R), *mmpos = ar.take<u32>(R + 1);
    u32 *ocnt = ar.take<u32>(R), *surv = ar.take<u32>(R), *newid = ar.take<u32>(R + 1), *ooff = ar.take<u32>(R + 1);
    RCCHK(ar.missing(c));
    CALLCHK(c, scan_launch(st, pass, n, ppos, sums, words + 6, 1, ppos + n));
    k_umi_reads<<<grid_n, TPB, 0, st>>>(rid, n, base, R, rstart);
    // 2. the molecules
    k_umi_keys<<<grid_r, TPB, 0, st>>>((const u64*)d_mol_key, R, k0, v0);
    CALLCHK(c, hipGetLastError());
    SortBufs s1{{k0, k1}, {v0, v1}};
    CALLCHK(c, radix_sort_pairs64(st, s1, R, ss));
    k_umi_heads<<<grid_r, TPB, 0, st>>>(s1.keys(), R, head);
    CALLCHK(c, scan_launch(st, head, R, hpos, sums, words + 7));
    RCCHK(c.read_back(back, words, 8));
    const u32 n_mols = (u32)back[7];
    k_umi_mols<<<grid_r, TPB, 0, st>>>(s1.keys(), s1.vals(), head, hpos, R, n_mols, isfirst, mstart, multi, words + 5);
    CALLCHK(c, scan_launch(st, multi, n_mols, mmpos, sums, words + 8));
    RCCHK(c.read_back(back, words, 9));
    const u32 n_multi = (u32)back[8];
    counts[5] = back[5];
    u32 *mm_first = ar.take<u32>(n_multi), *mm_size = ar.take<u32>(n_multi), *mrun = ar.take<u32>((u64)n_multi + 1);
    RCCHK(ar.missing(c));
    k_umi_assign<<<grid_r, TPB, 0, st>>>(s1.vals(), head, hpos, mstart, multi, mmpos, R, rmm, mm_first, mm_size);
    CALLCHK(c, hipGetLastError());
    // 3., 4. the intersections of the k > 1 molecules
    u32 *runstart = nullptr, *keep = nullptr, *kpos = nullptr;
    u64 n_runs = 0;
    SortBufs s2{{k0, k1}, {v0, v1}};
    const UmiKey kf(n_loci, n_haps);
    if (n_multi) {
        u32 *mark = ar.take<u32>(n), *cpos = ar.take<u32>(n + 1);
        RCCHK(ar.missing(c));
        k_umi_mark<<<grid_n, TPB, 0, st>>>(rid, pass, rmm, base, n, mark);
        CALLCHK(c, scan_launch(st, mark, n, cpos, sums, words + 9));
        RCCHK(c.read_back(back, words, 10));
        const u64 m = back[9];                                     // (at least two: every read starts on a passing record)
        u32 *dhead = ar.take<u32>(m), *dpos = ar.take<u32>(m + 1);
        RCCHK(ar.missing(c));
        k_umi_pairs<<<grid_n, TPB, 0, st>>>(rid, loc, hf, mark, cpos, rmm, base, n, kf, k0, v0);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, radix_sort_pairs64(st, s2, m, ss, kf.bits(n_multi)));
        const unsigned grid_m = nblk(m, UMI_WG_RECS);
        u32 *rhead = mark, *rpos = cpos;                           // (the compaction is done: m <= n)
        k_umi_runs<<<grid_m, TPB, 0, st>>>(s2.keys(), s2.vals(), m, rhead, dhead);
        CALLCHK(c, scan_launch(st, rhead, m, rpos, sums, words + 10));
        CALLCHK(c, scan_launch(st, dhead, m, dpos, sums, words + 11, 1, dpos + m));
        RCCHK(c.read_back(back, words, 12));
        n_runs = back[10];
        runstart = ar.take<u32>(n_runs + 1); kpos = ar.take<u32>(n_runs + 1);
        keep = dhead;                                              // (scanned: n_runs <= m)
        RCCHK(ar.missing(c));
        const unsigned grid_t = nblk(n_runs, UMI_WG_RECS);
        k_umi_runstart<<<grid_m, TPB, 0, st>>>(s2.keys(), rhead, rpos, m, (u32)n_runs, n_multi, kf, runstart, mrun);
        k_umi_keep<<<grid_t, TPB, 0, st>>>(s2.keys(), runstart, dpos, mm_size, (u32)n_runs, kf, keep);
        CALLCHK(c, scan_launch(st, keep, n_runs, kpos, sums, words + 12, 1, kpos + n_runs));
    }
    // 5. the sizes, then the outputs
    k_umi_counts<<<grid_r, TPB, 0, st>>>(isfirst, rmm, rstart, ppos, mrun, kpos, R, ocnt, surv);
    CALLCHK(c, scan_launch(st, surv, R, newid, sums, words + 13));
    CALLCHK(c, scan_launch(st, ocnt, R, ooff, sums, words + 14));
    RCCHK(c.read_back(back, words, 15));
    const u64 n_surv = back[13], n_out = back[14];
    if (n_out > n || n_surv > n_mols) return fail(nullptr, ECB_ERR_HIP, "umi: more records out than in (internal)");
    k_umi_emit_single<<<grid_n, TPB, 0, st>>>(rid, loc, hf, pass, ppos, rstart, rmm, newid, ooff, base, n, orid, oloc, ohf);
    if (n_runs) k_umi_emit_multi<<<nblk(n_runs, UMI_WG_RECS), TPB, 0, st>>>(s2.keys(), runstart, keep, kpos, mrun, mm_first, newid, ooff, (u32)n_runs, kf, orid, oloc, ohf);
    k_umi_first<<<grid_r, TPB, 0, st>>>(surv, newid, R, (u32*)d_out_first_read);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, hipStreamSynchronize(st));
    counts[1] = n_mols; counts[2] = n_multi; counts[3] = n_mols - n_surv; counts[4] = n_out;
    memcpy(out_counts, counts, sizeof counts);
    return ECB_OK;
}

extern "C" int ecb_collapse_umis(int device, const uint32_t* read_id, const uint32_t* locus, const uint32_t* hapflag, const uint64_t* mol_key, uint64_t n,
                                 uint64_t n_reads, uint32_t n_loci, uint32_t n_haps, uint32_t* out_read_id, uint32_t* out_locus, uint32_t* out_hapflag,
                                 uint32_t* out_first_read, uint64_t* out_counts) {
    RCCHK(umi_check_args(read_id, locus, hapflag, mol_key, n, n_reads, n_loci, n_haps, out_read_id, out_locus, out_hapflag, out_first_read, out_counts));
    Call c(device, "umi: "); if (c.rc) return c.rc;
    // (n_reads is not yet known to be the stream's: what is staged of the per-read arrays stops at n entries, which a stream cannot exceed)
    const u64 nr = std::min<u64>(n_reads, n);
    DevBuf<> di, dl, df, dk, oi, ol, of, ofr;
    RCCHK(stage_in(c, {{&di, read_id, n * 4}, {&dl, locus, n * 4}, {&df, hapflag, n * 4}, {&dk, mol_key, nr * 8}, {&oi, nullptr, n * 4}, {&ol, nullptr, n * 4},
                       {&of, nullptr, n * 4}, {&ofr, nullptr, nr * 4}}));
    RCCHK(ecb_collapse_umis_device(device, di.p, dl.p, df.p, dk.p, n, n_reads, n_loci, n_haps, oi.p, ol.p, of.p, ofr.p, out_counts));
    const u64 n_out = out_counts[4], n_surv = out_counts[1] - out_counts[3];
    return stage_out(c, {{out_read_id, &oi, n_out * 4}, {out_locus, &ol, n_out * 4}, {out_hapflag, &of, n_out * 4}, {out_first_read, &ofr, n_surv * 4}});
}
