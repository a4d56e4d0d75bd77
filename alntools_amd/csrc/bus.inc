// ---- bus2ec: the rows and cell counts of a multisample .bin from the records of a kallisto BUS file (ecb_bus_molecules /
// ecb_bus_molecules_device; included by ecb.hip after the salmon section, whose per-row sort-and-fold kernels it shares) ------------------------
// bustools count's rule for EC matrices (include/ecb_bus.h).  Every step is a map over an array, one of the library's scans
// (scan_launch), or its stable LSD sort (radix_sort_pairs64 with the bits named); nothing is placed by an atomic, so every output is a
// function of the input alone.  The only atomics are the atomicMin of the lowest offender and an atomicOr of error bits, which only a
// refusal reads.
//   1. k_bus_lines, k_sl_targets, k_bus_keep, k_bus_check: matrix.ec, the target map, the keep list and every record checked; the lowest
//      offending line and record by an atomicMin of (index << 8 | reason).  || read back: refusals
//   2. cells.  No keep list: barcodes sorted with their record index, k_run_heads + scan: a record's cell is the number of heads before
//      it (k_bus_cells).  A keep list: k_bus_check bisected it and flagged the entries seen; their scan numbers the cells
//      (k_bus_cells_keep), and a record of a barcode not kept gets the cell n_cells: it sorts last and no kernel takes it.
//   3. order (UMI mode).  A sort on ec, then a sort on (cell << 32 | UMI): the sort is stable, so the records come out by (cell, UMI, ec).
//   4. molecules.  k_bus_heads: heads of (cell, UMI) and, within them, of ec; two scans number the molecules and the distinct (molecule,
//      ec) pairs; k_bus_mols lays a molecule's distinct ECs side by side (mstart, de).  k = mstart[m + 1] - mstart[m].
//   5. intersection of the k > 1 molecules (k_bus_multi + scan lists them).  k_bus_cand: the shortest of the molecule's lines is the
//      candidate list (the first of equals).  Every candidate is looked up in the other k - 1 lines (bus_has: a walk for lines up to
//      BUS_MERGE_LEN, a bisection beyond).  candidates x (k - 1) below BUS_WAVE_WORK: one lane per molecule (k_bus_inter); from there on
//      one wave per molecule, a candidate per lane, placed by ballot (k_bus_inter_wave).  Each runs twice: a count, a scan, then the emit.
//   6. events.  k_bus_events: a k = 1 molecule is (cell, line), a surviving k > 1 molecule (cell, n_ecs + its rank among the survivors);
//      no-UMI: k_bus_events_raw, every record (cell, line) with its count.  Sorted on (cell, code); k_bus_nheads + scan + k_bus_nfold: the
//      runs summed in 64 bits -> N.  The codes are ascending in the final row numbers, so N's rows are too.
//   7. rows.  The lines that got an event, scanned, then the survivors; their lengths scanned; k_bus_pairs: every (row, target) becomes
//      (row << 32 | column << 5 | haplotype, 1 << haplotype), as in salmon2ec, and goes through its sort, k_sl_heads, scan, k_sl_emit and
//      k_sl_rowptr.
//   Every size is known before the first output is written: a capacity too small writes nothing.
namespace {
constexpr u32 BUS_MAX_UMILEN = ECB_BUS_MAX_UMILEN;   // the UMI's 2 bits per base must fit the low half of the (cell, UMI) sort key
constexpr u32 BUS_WAVE_WORK = 128;                   // candidates x (k - 1) from which a molecule's intersection is a wave's work, not a lane's
constexpr u32 BUS_MERGE_LEN = 8;                     // a line up to this long is walked, a longer one bisected (bus_has)
constexpr u32 BUS_NONE = 0xFFFFFFFFu;
enum : u32 { BUS_R_EC = 1, BUS_R_BARCODE, BUS_R_UMI };
enum : u32 { BUS_L_PTR = 1, BUS_L_TARGET, BUS_L_ORDER };
enum : u32 { BUS_E_KEEP = 1u, BUS_E_COUNT = 2u };
// a record as it lies in the file (the caller's pointer may have any alignment)
struct __attribute__((packed)) BusRec { u64 barcode, umi; int ec; u32 count, flags, pad; };
static_assert(sizeof(BusRec) == 32, "a BUS record is 32 bytes");

const char* bus_record_reason(u32 r) {
    switch (r) {
    case BUS_R_EC: return "ec below 0 or at or beyond the number of matrix.ec lines";
    case BUS_R_BARCODE: return "a barcode bit at or above 2 x bclen";
    case BUS_R_UMI: return "a UMI bit at or above 2 x umilen";
    default: return "unknown";
    }
}
const char* bus_line_reason(u32 r) {
    switch (r) {
    case BUS_L_PTR: return "line pointers that do not run from 0 to the number of target ids without falling";
    case BUS_L_TARGET: return "a target id at or beyond the number of targets";
    case BUS_L_ORDER: return "target ids not strictly ascending";
    default: return "unknown";
    }
}
// the last r of [0, n) with off[r] <= p (off[0] <= p)
__device__ __forceinline__ u32 bus_row_of(const u32* off, u32 n, u32 p) {
    u32 lo = 0, hi = n;
    while (lo + 1 < hi) { const u32 mid = lo + (hi - lo) / 2; if (off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
// whether the ascending ids [lo, hi) hold t
__device__ __forceinline__ bool bus_has(const u32* ids, u32 lo, u32 hi, u32 t) {
    if (hi - lo <= BUS_MERGE_LEN) {
        for (u32 j = lo; j < hi; ++j) { const u32 v = ids[j]; if (v >= t) return v == t; }
        return false;
    }
    const u32 end = hi;
    while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; if (ids[mid] < t) lo = mid + 1; else hi = mid; }
    return lo < end && ids[lo] == t;
}
// matrix.ec: thread l <= n_ecs its pointers, thread j < nt target id j
__global__ __launch_bounds__(TPB) void k_bus_lines(const u32* ptr, u32 n_ecs, const u32* ids, u64 nt, u32 n_targets, u64* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i <= n_ecs) {
        if (i == 0 && ptr[0] != 0u) offender(err, 0, BUS_L_PTR);
        if (i < n_ecs && ptr[i] > ptr[i + 1]) offender(err, i, BUS_L_PTR);
        if (i == n_ecs && (u64)ptr[i] != nt) offender(err, n_ecs ? n_ecs - 1 : 0, BUS_L_PTR);
    }
    if (i >= nt || !n_ecs) return;
    u32 l = bus_row_of(ptr, n_ecs + 1, (u32)i);                 // (on pointers that fall this is some line; those are refused first)
    if (l >= n_ecs) l = n_ecs - 1;
    const u32 t = ids[i];
    if (t >= n_targets) offender(err, l, BUS_L_TARGET);
    if (i + 1 < nt && i + 1 < (u64)ptr[l + 1] && ids[i + 1] <= t) offender(err, l, BUS_L_ORDER);
}
__global__ __launch_bounds__(TPB) void k_bus_keep(const u64* keep, u64 n_keep, u32* bits) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j + 1 < n_keep && keep[j] >= keep[j + 1]) atomicOr(bits, BUS_E_KEEP);
}
// record i checked.  No keep list: (barcode, i) for the sort.  A keep list: the record's place in it (BUS_NONE: not kept), the place flagged
__global__ __launch_bounds__(TPB) void k_bus_check(const BusRec* recs, u64 n, u32 bcbits, u32 umibits, u32 n_ecs, const u64* keep, u64 n_keep, u64* err,
                                                   u64* keys, u32* vals, u32* kidx, u32* present) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u64 bc = recs[i].barcode, umi = recs[i].umi;
    const int ec = recs[i].ec;
    if (ec < 0 || (u32)ec >= n_ecs) offender(err, i, BUS_R_EC);
    else if (bcbits < 64u && (bc >> bcbits)) offender(err, i, BUS_R_BARCODE);
    else if (umibits < 64u && (umi >> umibits)) offender(err, i, BUS_R_UMI);
    if (!keep) { keys[i] = bc; vals[i] = (u32)i; return; }
    const u64 q = lower_bound_u64(keep, n_keep, bc);
    const bool in = q < n_keep && keep[q] == bc;
    kidx[i] = in ? (u32)q : BUS_NONE;
    if (in) present[q] = 1u;                                  // (every writer stores the same word)
}
// sorted barcodes: the cell of every record, and the barcode of every cell
__global__ __launch_bounds__(TPB) void k_bus_cells(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u32* cell, u64* barcodes) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n) return;
    const u32 c = pos[j] + flag[j] - 1u;                        // (pos: heads before j)
    cell[vals[j]] = c;
    if (flag[j]) barcodes[c] = keys[j];
}
__global__ __launch_bounds__(TPB) void k_bus_cells_keep(const u32* kidx, u64 n, const u32* kpos, u32 n_cells, u32* cell) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) cell[i] = kidx[i] == BUS_NONE ? n_cells : kpos[kidx[i]];
}
__global__ __launch_bounds__(TPB) void k_bus_keep_barcodes(const u64* keep, u64 n_keep, const u32* present, const u32* kpos, u64* barcodes) {
    const u64 q = blockIdx.x * (u64)TPB + threadIdx.x;
    if (q < n_keep && present[q]) barcodes[kpos[q]] = keep[q];
}
__global__ __launch_bounds__(TPB) void k_bus_eckeys(const BusRec* recs, u64 n, u64* keys, u32* vals) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) { keys[i] = (u64)(u32)recs[i].ec; vals[i] = (u32)i; }
}
// place j of the ec order: (cell << 32 | UMI) of its record, in place
__global__ __launch_bounds__(TPB) void k_bus_molkeys(const BusRec* recs, const u32* cell, u64 n, u64* keys, const u32* vals) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j < n) { const u32 i = vals[j]; keys[j] = (u64)cell[i] << 32 | (u64)(u32)recs[i].umi; }
}
// sorted by (cell, UMI, ec): the ec of every place; heads of the molecules and of the distinct ECs within them (none for a record not kept)
__global__ __launch_bounds__(TPB) void k_bus_heads(const BusRec* recs, const u64* keys, const u32* vals, u64 n, u32 n_cells, u32* ecs, u32* mhead, u32* ehead) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n) return;
    const u64 k = keys[j];
    const u32 e = (u32)recs[vals[j]].ec;
    ecs[j] = e;
    const bool valid = (u32)(k >> 32) < n_cells;
    const bool mh = valid && (j == 0 || keys[j - 1] != k);
    mhead[j] = mh;
    ehead[j] = valid && (mh || (u32)recs[vals[j - 1]].ec != e);
}
__global__ __launch_bounds__(TPB) void k_bus_mols(const u64* keys, const u32* ecs, const u32* mhead, const u32* ehead, const u32* mpos, const u32* epos, u64 n,
                                                  u32 n_mols, u32 n_des, u32* mstart, u32* mcell, u32* de) {
    const u64 j = blockIdx.x * (u64)TPB + threadIdx.x;
    if (j >= n) return;
    if (j == 0) mstart[n_mols] = n_des;
    if (mhead[j]) { mstart[mpos[j]] = epos[j]; mcell[mpos[j]] = (u32)(keys[j] >> 32); }
    if (ehead[j]) de[epos[j]] = ecs[j];
}
__global__ __launch_bounds__(TPB) void k_bus_multi(const u32* mstart, u32 n_mols, u32* multi) {
    const u64 m = blockIdx.x * (u64)TPB + threadIdx.x;
    if (m < n_mols) multi[m] = mstart[m + 1] - mstart[m] > 1u;
}
// the k > 1 molecules listed; of each the candidate list: the place in de of its shortest line (the first of equals) and that length
__global__ __launch_bounds__(TPB) void k_bus_cand(const u32* mstart, const u32* multi, const u32* mmpos, u32 n_mols, const u32* de, const u32* ptr, u32* mm_mol,
                                                  u32* cand, u32* clen) {
    const u64 m = blockIdx.x * (u64)TPB + threadIdx.x;
    if (m >= n_mols || !multi[m]) return;
    const u32 a = mstart[m], b = mstart[m + 1];
    u32 best = a, bl = ptr[de[a] + 1] - ptr[de[a]];
    for (u32 q = a + 1; q < b; ++q) { const u32 l = ptr[de[q] + 1] - ptr[de[q]]; if (l < bl) { bl = l; best = q; } }
    const u32 mm = mmpos[m];
    mm_mol[mm] = (u32)m; cand[mm] = best; clen[mm] = bl;
}
__device__ __forceinline__ bool bus_wave_path(u32 clen, u32 k) { return (u64)clen * (k - 1u) >= BUS_WAVE_WORK; }
// whether target t is in every line of de[a, b) but the one at `skip`
__device__ __forceinline__ bool bus_in_all(const u32* de, u32 a, u32 b, u32 skip, const u32* ptr, const u32* ids, u32 t) {
    for (u32 q = a; q < b; ++q) {
        if (q == skip) continue;
        const u32 e = de[q];
        if (!bus_has(ids, ptr[e], ptr[e + 1], t)) return false;
    }
    return true;
}
// one lane per k > 1 molecule.  EMIT false: cnt[mm]; true: the targets at inter[ioff[mm] ..)
template <bool EMIT>
__global__ __launch_bounds__(TPB) void k_bus_inter(const u32* mm_mol, const u32* cand, const u32* clen, u32 n_multi, const u32* mstart, const u32* de,
                                                   const u32* ptr, const u32* ids, u32* cnt, const u32* ioff, u32* inter) {
    const u64 mm = blockIdx.x * (u64)TPB + threadIdx.x;
    if (mm >= n_multi) return;
    const u32 m = mm_mol[mm], a = mstart[m], b = mstart[m + 1], len = clen[mm];
    if (bus_wave_path(len, b - a)) return;
    const u32 best = cand[mm], c0 = ptr[de[best]];
    u32 count = 0;
    for (u32 c = 0; c < len; ++c) {
        const u32 t = ids[c0 + c];
        if (!bus_in_all(de, a, b, best, ptr, ids, t)) continue;
        if (EMIT) inter[ioff[mm] + count] = t;
        ++count;
    }
    if (!EMIT) cnt[mm] = count;
}
// one wave per k > 1 molecule of the wave path: a candidate per lane, the hits placed in order by ballot
template <bool EMIT>
__global__ __launch_bounds__(TPB) void k_bus_inter_wave(const u32* mm_mol, const u32* cand, const u32* clen, u32 n_multi, const u32* mstart, const u32* de,
                                                        const u32* ptr, const u32* ids, u32* cnt, const u32* ioff, u32* inter) {
    const u64 mm = blockIdx.x * (u64)(TPB / 64) + (threadIdx.x >> 6);
    if (mm >= n_multi) return;
    const u32 lane = threadIdx.x & 63u;
    const u32 m = mm_mol[mm], a = mstart[m], b = mstart[m + 1], len = clen[mm];
    if (!bus_wave_path(len, b - a)) return;
    const u32 best = cand[mm], c0 = ptr[de[best]];
    u32 count = 0;
    for (u32 base = 0; base < len; base += 64u) {
        const u32 c = base + lane;
        u32 t = 0;
        bool hit = false;
        if (c < len) { t = ids[c0 + c]; hit = bus_in_all(de, a, b, best, ptr, ids, t); }
        const u64 hits = __ballot(hit);
        if (EMIT && hit) inter[ioff[mm] + count + (u32)__popcll(hits & ((1ull << lane) - 1ull))] = t;
        count += (u32)__popcll(hits);
    }
    if (!EMIT && lane == 0u) cnt[mm] = count;
}
__global__ __launch_bounds__(TPB) void k_bus_surv(const u32* cnt, u32 n_multi, u32* surv) {
    const u64 mm = blockIdx.x * (u64)TPB + threadIdx.x;
    if (mm < n_multi) surv[mm] = cnt[mm] != 0u;
}
// molecule m: its event (cell << 32 | code, 1): code = the line of a k = 1 molecule (flagged as used), n_ecs + rank of a survivor; a
// discarded molecule gets the cell n_cells.  The survivors listed
__global__ __launch_bounds__(TPB) void k_bus_events(const u32* mstart, const u32* mcell, const u32* de, const u32* multi, const u32* mmpos, const u32* surv,
                                                    const u32* spos, u32 n_mols, u32 n_ecs, u32 n_cells, u64* keys, u32* vals, u32* used, u32* surv_mm) {
    const u64 m = blockIdx.x * (u64)TPB + threadIdx.x;
    if (m >= n_mols) return;
    u64 key = (u64)n_cells << 32;
    if (!multi[m]) {
        const u32 e = de[mstart[m]];
        key = (u64)mcell[m] << 32 | e;
        used[e] = 1u;
    } else {
        const u32 mm = mmpos[m];
        if (surv[mm]) { key = (u64)mcell[m] << 32 | ((u64)n_ecs + spos[mm]); surv_mm[spos[mm]] = mm; }
    }
    keys[m] = key; vals[m] = 1u;
}
// no-UMI: record i is `count` reads of its line in its cell
__global__ __launch_bounds__(TPB) void k_bus_events_raw(const BusRec* recs, const u32* cell, u64 n, u32 n_cells, u64* keys, u32* vals, u32* used) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    const u32 c = cell[i], e = (u32)recs[i].ec, w = recs[i].count;
    const bool counts = c < n_cells && w != 0u;
    keys[i] = counts ? (u64)c << 32 | e : (u64)n_cells << 32;
    vals[i] = w;
    if (counts) used[e] = 1u;
}
__global__ __launch_bounds__(TPB) void k_bus_nheads(const u64* keys, u64 n, u32 n_cells, u32* flag) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) flag[i] = (u32)(keys[i] >> 32) < n_cells && (i == 0 || keys[i - 1] != keys[i]);
}
// a run of equal (cell, code): its counts summed in 64 bits
__global__ __launch_bounds__(TPB) void k_bus_nfold(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u64 n, u32* code, u32* sum, u32* bits) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u64 k = keys[i];
    u64 s = 0;
    for (u64 j = i; j < n && keys[j] == k; ++j) s += vals[j];
    if (s > 0x7FFFFFFFull) { atomicOr(bits, BUS_E_COUNT); s = 0x7FFFFFFFull; }
    code[pos[i]] = (u32)k; sum[pos[i]] = (u32)s;
}
__global__ __launch_bounds__(TPB) void k_bus_line_rows(const u32* used, const u32* lrow, u32 n_ecs, u32* line_of_row) {
    const u64 l = blockIdx.x * (u64)TPB + threadIdx.x;
    if (l < n_ecs && used[l]) line_of_row[lrow[l]] = (u32)l;
}
__global__ __launch_bounds__(TPB) void k_bus_rowlen(const u32* line_of_row, u32 n_line_rows, const u32* surv_mm, const u32* cnt, u32 n_rows, const u32* ptr, u32* len) {
    const u64 r = blockIdx.x * (u64)TPB + threadIdx.x;
    if (r >= n_rows) return;
    if (r < n_line_rows) { const u32 l = line_of_row[r]; len[r] = ptr[l + 1] - ptr[l]; }
    else len[r] = cnt[surv_mm[r - n_line_rows]];
}
// pair p: target q of row r -> salmon2ec's (row << 32 | column << 5 | haplotype, 1 << haplotype)
__global__ __launch_bounds__(TPB) void k_bus_pairs(const u32* rowoff, u32 n_rows, u32 n_line_rows, const u32* line_of_row, const u32* surv_mm, const u32* ioff,
                                                   const u32* inter, const u32* ptr, const u32* ids, const u32* tcol, const u32* thap, u64 np, u64* keys, u32* vals) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x;
    if (p >= np) return;
    const u32 r = bus_row_of(rowoff, n_rows + 1, (u32)p), q = (u32)p - rowoff[r];
    const u32 t = r < n_line_rows ? ids[ptr[line_of_row[r]] + q] : inter[ioff[surv_mm[r - n_line_rows]] + q];
    const u32 h = thap[t];
    keys[p] = (u64)r << 32 | (tcol[t] << 5 | h);
    vals[p] = 1u << h;
}
__global__ __launch_bounds__(TPB) void k_bus_row_line(const u32* line_of_row, u32 n_line_rows, u32 n_rows, int* row_line) {
    const u64 r = blockIdx.x * (u64)TPB + threadIdx.x;
    if (r < n_rows) row_line[r] = r < n_line_rows ? (int)line_of_row[r] : -1;
}
// N: the folded runs with their final row numbers; the column pointers by bisection of the sorted events
__global__ __launch_bounds__(TPB) void k_bus_n_out(const u32* code, const u32* sum, u64 nn, const u32* lrow, u32 n_ecs, u32 n_line_rows, const u64* keys,
                                                   const u32* pos, u64 n_events, u32 n_cells, int* indptr, int* indices, int* data) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < nn) { const u32 c = code[i]; indices[i] = (int)(c < n_ecs ? lrow[c] : n_line_rows + (c - n_ecs)); data[i] = (int)sum[i]; }
    if (i <= n_cells) indptr[i] = (int)pos[lower_bound_u64(keys, n_events, i << 32)];
}
__global__ __launch_bounds__(TPB) void k_bus_count_events(const u64* keys, u64 n_events, u32 n_cells, u64* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = lower_bound_u64(keys, n_events, (u64)n_cells << 32);
}

int bus_check_args(const void* records, uint64_t n, uint32_t bclen, uint32_t umilen, uint32_t flags, uint32_t n_ecs, uint64_t nt, const void* ec_ptr,
                   const void* ec_targets, uint32_t n_targets, const void* tcol, const void* thap, uint32_t n_loci, uint32_t n_haps, const void* keep,
                   uint64_t n_keep, uint64_t cap_cells, uint64_t cap_rows, uint64_t cap_a, uint64_t cap_n, const void* ob, const void* oipa, const void* oixa,
                   const void* odaa, const void* oipn, const void* oixn, const void* odn, const void* orl, const void* out_sizes) {
    if (!records || !n || !n_ecs || !ec_ptr || (nt && !ec_targets) || !n_targets || !tcol || !thap || !n_loci || !n_haps || n_haps > 31 || !out_sizes ||
        (n_keep && !keep) || !oipa || !oipn || (cap_cells && !ob) || (cap_rows && !orl) || (cap_a && (!oixa || !odaa)) || (cap_n && (!oixn || !odn)))
        return fail(nullptr, ECB_ERR_ARG, "bus: bad argument");
    if (flags & ~ECB_BUS_NO_UMI) return fail(nullptr, ECB_ERR_ARG, "bus: unknown flag bits");
    if (bclen < 1 || bclen > 32 || umilen < 1 || umilen > 32) return fail(nullptr, ECB_ERR_ARG, "bus: bclen and umilen are 1 .. 32");
    if (n_loci >= MAX_LOCI) return fail(nullptr, ECB_ERR_ARG, "bus: n_loci out of range (1 .. 2^26-3)");
    if (!(flags & ECB_BUS_NO_UMI) && umilen > BUS_MAX_UMILEN)
        return fail(nullptr, ECB_ERR_LIMIT, "bus: a UMI of %u bases; the (cell, UMI) sort key holds %u", umilen, BUS_MAX_UMILEN);
    if (n >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "bus: 2^30 records or more");                   // (radix_sort_pairs64)
    if (n_ecs >= (1u << 31) || nt >= (1ull << 32) || n_targets >= (1u << 31) || n_keep >= (1ull << 32))
        return fail(nullptr, ECB_ERR_LIMIT, "bus: matrix.ec, the targets or the keep list beyond 32 bits");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_bus_molecules_device(int device, const void* d_records, uint64_t n, uint32_t bclen, uint32_t umilen, uint32_t flags, uint32_t n_ecs,
                                        uint64_t n_ec_targets, const void* d_ec_ptr, const void* d_ec_targets, uint32_t n_targets, const void* d_target_col,
                                        const void* d_target_hap, uint32_t n_loci, uint32_t n_haps, const void* d_keep, uint64_t n_keep, uint64_t cap_cells,
                                        uint64_t cap_rows, uint64_t cap_a, uint64_t cap_n, void* d_out_barcodes, void* d_out_indptr_a, void* d_out_indices_a,
                                        void* d_out_data_a, void* d_out_indptr_n, void* d_out_indices_n, void* d_out_data_n, void* d_out_row_line,
                                        uint64_t* out_sizes) {
    RCCHK(bus_check_args(d_records, n, bclen, umilen, flags, n_ecs, n_ec_targets, d_ec_ptr, d_ec_targets, n_targets, d_target_col, d_target_hap, n_loci,
                         n_haps, d_keep, n_keep, cap_cells, cap_rows, cap_a, cap_n, d_out_barcodes, d_out_indptr_a, d_out_indices_a, d_out_data_a,
                         d_out_indptr_n, d_out_indices_n, d_out_data_n, d_out_row_line, out_sizes));
    Call c(device, "bus: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const bool no_umi = flags & ECB_BUS_NO_UMI;
    const BusRec* recs = (const BusRec*)d_records;
    const u32 *ptr = (const u32*)d_ec_ptr, *ids = (const u32*)d_ec_targets, *tcol = (const u32*)d_target_col, *thap = (const u32*)d_target_hap;
    const u64* keep = (const u64*)d_keep;
    const u32 bcbits = 2 * bclen, umibits = 2 * umilen;
    const u64 nt = n_ec_targets;
    // the sort's buffers are the device's pool's (one sort at a time lives in them); what has to outlive a sort is cut from one more pool
    // buffer (Arena), the intersections and the rows' flags, whose sizes the data decides, from three others
    u64 *k0 = nullptr, *k1 = nullptr;
    u32 *v0 = nullptr, *v1 = nullptr;
    SortScratch ss{};
    // [0] lowest (line << 8 | reason)  [1] lowest (record << 8 | reason)  [2] error bits  [3] the sort's word  [4 ..) scan totals
    u64* words;
    RCCHK(c.status_words(words, 16, 2));
    auto sort_room = [&](u64 m) {
        k0 = c.get<u64>(CV_KEYS0, m); k1 = c.get<u64>(CV_KEYS1, m); v0 = c.get<u32>(CV_VALS0, m); v1 = c.get<u32>(CV_VALS1, m);
        ss = SortScratch{c.get<u32>(CV_HIST, rs_words(m)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 3};
        return c.missing();
    };
    // the arena's room: every buffer below at its bound -- molecules, distinct (molecule, ec) pairs, events and rows are at most n, the
    // molecules of several ECs at most n / 2
    const u64 nk = keep ? n_keep : 0, e1 = (u64)n_ecs + 1, half = n / 2 + 2;
    const auto pad = Arena::pad;
    Arena ar(c, CV_X0, 6 * pad(n + 1, 4) + pad(n, 8) + (keep ? pad(n, 4) + 2 * pad(nk + 1, 4) : 0) + 2 * pad(e1, 4) +
                           pad(scan_words(std::max<u64>(std::max<u64>(n, nk), e1)), 4) + (no_umi ? 0 : 5 * pad(n + 1, 4) + 8 * pad(half, 4)) +
                           3 * pad(n + 1, 4) + pad(n, 8) + 3 * pad(n + 1, 4) + pad(scan_words(n + 1), 4));
    RCCHK(c.missing());
    u32* cell = ar.take<u32>(n);
    u32 *flag = ar.take<u32>(n), *flag2 = ar.take<u32>(n), *pos = ar.take<u32>(n + 1), *pos2 = ar.take<u32>(n + 1), *ecs = ar.take<u32>(n);
    u64* barcodes = ar.take<u64>(keep ? std::min<u64>(n, n_keep) : n);
    u32 *kidx = nullptr, *present = nullptr, *kpos = nullptr;
    if (keep) { kidx = ar.take<u32>(n); present = ar.take<u32>(n_keep); kpos = ar.take<u32>(n_keep + 1); }
    u32 *used = ar.take<u32>(n_ecs), *lrow = ar.take<u32>((u64)n_ecs + 1);
    u32* sums = ar.take<u32>(scan_words(std::max<u64>(std::max<u64>(n, n_keep), (u64)n_ecs + 1)));
    RCCHK(ar.missing(c));
    RCCHK(sort_room(n));
    u64 back[16];
    u32* bits = reinterpret_cast<u32*>(words + 2);
    CALLCHK(c, hipMemsetAsync(used, 0, (u64)n_ecs * 4, st));
    if (keep) CALLCHK(c, hipMemsetAsync(present, 0, std::max<u64>(n_keep, 1) * 4, st));
    // 1. the checks
    k_bus_lines<<<nblk(std::max<u64>((u64)n_ecs + 1, nt), TPB), TPB, 0, st>>>(ptr, n_ecs, ids, nt, n_targets, words);
    k_sl_targets<<<nblk(n_targets, TPB), TPB, 0, st>>>(tcol, thap, n_targets, n_loci, n_haps, bits + 1);
    if (n_keep > 1) k_bus_keep<<<nblk(n_keep, TPB), TPB, 0, st>>>(keep, n_keep, bits);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words, 4));
    RCCHK(refuse_offender(back[0], "bus: matrix.ec line", bus_line_reason));      // (the records name lines: not looked at before matrix.ec stands)
    if (back[2] >> 32) return fail(nullptr, ECB_ERR_CONTRACT, "bus: the target map has a column at or beyond n_loci or a haplotype at or beyond n_haps");
    if ((u32)back[2] & BUS_E_KEEP) return fail(nullptr, ECB_ERR_CONTRACT, "bus: the barcodes to keep are not strictly ascending");
    k_bus_check<<<nblk(n, TPB), TPB, 0, st>>>(recs, n, bcbits, umibits, n_ecs, keep, n_keep, words + 1, k0, v0, kidx, present);
    CALLCHK(c, hipGetLastError());
    RCCHK(c.read_back(back, words, 4));
    RCCHK(refuse_offender(back[1], "bus: record", bus_record_reason));
    // 2. the cells
    u64 n_cells64 = 0;
    if (!keep) {
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, n, ss, bcbits < 64u ? (1ull << bcbits) - 1ull : ~0ull));
        k_run_heads<<<nblk(n, TPB), TPB, 0, st>>>(s.keys(), n, flag);
        CALLCHK(c, scan_launch(st, flag, n, pos, sums, words + 4));
        k_bus_cells<<<nblk(n, TPB), TPB, 0, st>>>(s.keys(), s.vals(), flag, pos, n, cell, barcodes);
        CALLCHK(c, hipGetLastError());
        RCCHK(c.read_back(back, words, 8));
        n_cells64 = back[4];
    } else {
        CALLCHK(c, scan_launch(st, present, n_keep, kpos, sums, words + 4, 1, kpos + n_keep));
        RCCHK(c.read_back(back, words, 8));
        n_cells64 = back[4];
        k_bus_cells_keep<<<nblk(n, TPB), TPB, 0, st>>>(kidx, n, kpos, (u32)n_cells64, cell);
        if (n_keep) k_bus_keep_barcodes<<<nblk(n_keep, TPB), TPB, 0, st>>>(keep, n_keep, present, kpos, barcodes);
        CALLCHK(c, hipGetLastError());
    }
    const u32 n_cells = (u32)n_cells64;
    // 3. - 5. the molecules and their intersections (UMI mode); 6. the events
    u64 n_events = n, n_mols = 0, n_multi = 0, n_surv = 0;
    u32 *cnt = nullptr, *ioff = nullptr, *inter = nullptr, *surv_mm = nullptr;
    if (no_umi) {
        k_bus_events_raw<<<nblk(n, TPB), TPB, 0, st>>>(recs, cell, n, n_cells, k0, v0, used);
        CALLCHK(c, hipGetLastError());
    } else {
        k_bus_eckeys<<<nblk(n, TPB), TPB, 0, st>>>(recs, n, k0, v0);
        SortBufs s1{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s1, n, ss, msb_mask(n_ecs - 1)));
        k_bus_molkeys<<<nblk(n, TPB), TPB, 0, st>>>(recs, cell, n, s1.keys(), s1.vals());
        SortBufs s{{s1.keys(), s1.spare_keys()}, {s1.vals(), s1.spare_vals()}};
        CALLCHK(c, radix_sort_pairs64(st, s, n, ss, msb_mask(n_cells) << 32 | (umibits < 32u ? (1ull << umibits) - 1ull : 0xFFFFFFFFull)));
        k_bus_heads<<<nblk(n, TPB), TPB, 0, st>>>(recs, s.keys(), s.vals(), n, n_cells, ecs, flag, flag2);
        CALLCHK(c, scan_launch(st, flag, n, pos, sums, words + 5));
        CALLCHK(c, scan_launch(st, flag2, n, pos2, sums, words + 6));
        RCCHK(c.read_back(back, words, 8));
        n_mols = back[5];
        const u64 n_des = back[6];
        u32 *mstart = ar.take<u32>(n_mols + 1), *mcell = ar.take<u32>(n_mols), *de = ar.take<u32>(n_des), *multi = ar.take<u32>(n_mols), *mmpos = ar.take<u32>(n_mols + 1);
        RCCHK(ar.missing(c));
        k_bus_mols<<<nblk(n, TPB), TPB, 0, st>>>(s.keys(), ecs, flag, flag2, pos, pos2, n, (u32)n_mols, (u32)n_des, mstart, mcell, de);
        if (n_mols) k_bus_multi<<<nblk(n_mols, TPB), TPB, 0, st>>>(mstart, (u32)n_mols, multi);
        CALLCHK(c, scan_launch(st, multi, n_mols, mmpos, sums, words + 7));
        RCCHK(c.read_back(back, words, 8));
        n_multi = back[7];
        u32 *mm_mol = ar.take<u32>(n_multi), *cand = ar.take<u32>(n_multi), *clen = ar.take<u32>(n_multi), *surv = ar.take<u32>(n_multi), *spos = ar.take<u32>(n_multi + 1);
        cnt = ar.take<u32>(n_multi); ioff = ar.take<u32>(n_multi + 1); surv_mm = ar.take<u32>(n_multi);
        RCCHK(ar.missing(c));
        u64 n_inter = 0;
        if (n_multi) {
            const unsigned gl = nblk(n_multi, TPB), gw = nblk(n_multi, TPB / 64);
            k_bus_cand<<<nblk(n_mols, TPB), TPB, 0, st>>>(mstart, multi, mmpos, (u32)n_mols, de, ptr, mm_mol, cand, clen);
            k_bus_inter<false><<<gl, TPB, 0, st>>>(mm_mol, cand, clen, (u32)n_multi, mstart, de, ptr, ids, cnt, nullptr, nullptr);
            k_bus_inter_wave<false><<<gw, TPB, 0, st>>>(mm_mol, cand, clen, (u32)n_multi, mstart, de, ptr, ids, cnt, nullptr, nullptr);
            k_bus_surv<<<gl, TPB, 0, st>>>(cnt, (u32)n_multi, surv);
            CALLCHK(c, scan_launch(st, cnt, n_multi, ioff, sums, words + 8, 1, ioff + n_multi));
            CALLCHK(c, scan_launch(st, surv, n_multi, spos, sums, words + 9));
            RCCHK(c.read_back(back, words, 10));
            n_inter = back[8]; n_surv = back[9];
            if (n_inter >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "bus: 2^30 (row, target) pairs or more");
            inter = c.get<u32>(CV_X1, n_inter);
            RCCHK(c.missing());
            k_bus_inter<true><<<gl, TPB, 0, st>>>(mm_mol, cand, clen, (u32)n_multi, mstart, de, ptr, ids, nullptr, ioff, inter);
            k_bus_inter_wave<true><<<gw, TPB, 0, st>>>(mm_mol, cand, clen, (u32)n_multi, mstart, de, ptr, ids, nullptr, ioff, inter);
        }
        n_events = n_mols;
        if (n_mols) k_bus_events<<<nblk(n_mols, TPB), TPB, 0, st>>>(mstart, mcell, de, multi, mmpos, surv, spos, (u32)n_mols, n_ecs, n_cells, k0, v0, used, surv_mm);
        CALLCHK(c, hipGetLastError());
    }
    // ... sorted and folded: N, still in codes
    u32 *ncode = ar.take<u32>(n_events), *nsum = ar.take<u32>(n_events), *nkeys_pos = ar.take<u32>(n_events + 1);
    u64* ekeys = ar.take<u64>(n_events);
    RCCHK(ar.missing(c));
    {
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, n_events, ss, msb_mask(n_cells) << 32 | msb_mask((u64)n_ecs + n_surv)));
        k_bus_nheads<<<nblk(std::max<u64>(n_events, 1), TPB), TPB, 0, st>>>(s.keys(), n_events, n_cells, flag);
        CALLCHK(c, scan_launch(st, flag, n_events, nkeys_pos, sums, words + 10, 1, nkeys_pos + n_events));
        if (n_events) k_bus_nfold<<<nblk(n_events, TPB), TPB, 0, st>>>(s.keys(), s.vals(), flag, nkeys_pos, n_events, ncode, nsum, bits);
        k_bus_count_events<<<1, 64, 0, st>>>(s.keys(), n_events, n_cells, words + 11);
        CALLCHK(c, hipMemcpyAsync(ekeys, s.keys(), n_events * 8, hipMemcpyDeviceToDevice, st));      // (the pool's buffers go to the rows' sort next)
    }
    // 7. the rows
    CALLCHK(c, scan_launch(st, used, n_ecs, lrow, sums, words + 12, 1, lrow + n_ecs));
    RCCHK(c.read_back(back, words, 16));
    if ((u32)back[2] & BUS_E_COUNT) return fail(nullptr, ECB_ERR_LIMIT, "bus: the reads of one row in one cell add up beyond int32");
    const u64 nnz_n = back[10], n_counted = back[11], n_line_rows = back[12], n_rows = n_line_rows + n_surv;
    if (n_rows >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "bus: rows beyond int32");
    u32 *line_of_row = ar.take<u32>(n_line_rows), *rowlen = ar.take<u32>(n_rows), *rowoff = ar.take<u32>(n_rows + 1);
    u32* sums2 = ar.take<u32>(scan_words(n_rows));
    RCCHK(ar.missing(c));
    k_bus_line_rows<<<nblk(n_ecs, TPB), TPB, 0, st>>>(used, lrow, n_ecs, line_of_row);
    if (n_rows) k_bus_rowlen<<<nblk(n_rows, TPB), TPB, 0, st>>>(line_of_row, (u32)n_line_rows, surv_mm, cnt, (u32)n_rows, ptr, rowlen);
    CALLCHK(c, scan_launch(st, rowlen, n_rows, rowoff, sums2, words + 13, 1, rowoff + n_rows));
    RCCHK(c.read_back(back, words, 16));
    const u64 np = back[13];
    if (np >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "bus: 2^30 (row, target) pairs or more");
    RCCHK(sort_room(np));
    u32 *aflag = c.get<u32>(CV_X2, np), *apos = c.get<u32>(CV_X3, np + 1), *sums3 = c.get<u32>(CV_SUMS2, scan_words(np));
    RCCHK(c.missing());
    if (np) k_bus_pairs<<<nblk(np, TPB), TPB, 0, st>>>(rowoff, (u32)n_rows, (u32)n_line_rows, line_of_row, surv_mm, ioff, inter, ptr, ids, tcol, thap, np, k0, v0);
    SortBufs sa{{k0, k1}, {v0, v1}};
    CALLCHK(c, radix_sort_pairs64(st, sa, np, ss, msb_mask(n_rows ? n_rows - 1 : 0) << 32 | msb_mask((u64)(n_loci - 1) << 5 | 31u)));
    CALLCHK(c, hipMemsetAsync(words + 14, 0xFF, 8, st));
    if (np) k_sl_heads<<<nblk(np, TPB), TPB, 0, st>>>(sa.keys(), np, aflag, words + 14);
    CALLCHK(c, scan_launch(st, aflag, np, apos, sums3, words + 15, 1, apos + np));
    RCCHK(c.read_back(back, words, 16));
    if (back[14] != NO_OFFENDER) return fail(nullptr, ECB_ERR_CONTRACT, "bus: two targets of row %llu share a (column, haplotype)", (unsigned long long)(back[14] >> 8));
    const u64 nnz_a = np ? back[15] : 0;
    if (nnz_a >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "bus: non-zeros beyond int32");
    // every size is known: the capacities, then the outputs
    if (n_cells64 > cap_cells || n_rows > cap_rows || nnz_a > cap_a || nnz_n > cap_n)
        return fail(nullptr, ECB_ERR_ARG, "bus: %llu cells, %llu rows, %llu and %llu non-zeros of A and N; room for %llu, %llu, %llu and %llu",
                    (unsigned long long)n_cells64, (unsigned long long)n_rows, (unsigned long long)nnz_a, (unsigned long long)nnz_n,
                    (unsigned long long)cap_cells, (unsigned long long)cap_rows, (unsigned long long)cap_a, (unsigned long long)cap_n);
    if (n_cells) CALLCHK(c, hipMemcpyAsync(d_out_barcodes, barcodes, n_cells64 * 8, hipMemcpyDeviceToDevice, st));
    if (np) k_sl_emit<<<nblk(np, TPB), TPB, 0, st>>>(sa.keys(), sa.vals(), aflag, apos, np, cap_a, (int*)d_out_indices_a, (int*)d_out_data_a);
    k_sl_rowptr<<<nblk(n_rows + 1, TPB), TPB, 0, st>>>(sa.keys(), np, apos, (u32)n_rows, (int*)d_out_indptr_a);
    if (n_rows) k_bus_row_line<<<nblk(n_rows, TPB), TPB, 0, st>>>(line_of_row, (u32)n_line_rows, (u32)n_rows, (int*)d_out_row_line);
    k_bus_n_out<<<nblk(std::max<u64>(nnz_n, n_cells64 + 1), TPB), TPB, 0, st>>>(ncode, nsum, nnz_n, lrow, n_ecs, (u32)n_line_rows, ekeys, nkeys_pos, n_events, n_cells,
                                                                             (int*)d_out_indptr_n, (int*)d_out_indices_n, (int*)d_out_data_n);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, hipStreamSynchronize(st));
    const u64 sizes[8] = {n_cells64, n_rows, nnz_a, nnz_n, no_umi ? n_counted : n_mols, n_multi, n_multi - n_surv, n_surv};
    memcpy(out_sizes, sizes, sizeof sizes);
    return ECB_OK;
}

extern "C" int ecb_bus_molecules(int device, const void* records, uint64_t n, uint32_t bclen, uint32_t umilen, uint32_t flags, uint32_t n_ecs,
                                 uint64_t n_ec_targets, const uint32_t* ec_ptr, const uint32_t* ec_targets, uint32_t n_targets, const uint32_t* target_col,
                                 const uint32_t* target_hap, uint32_t n_loci, uint32_t n_haps, const uint64_t* keep, uint64_t n_keep, uint64_t cap_cells,
                                 uint64_t cap_rows, uint64_t cap_a, uint64_t cap_n, uint64_t* out_barcodes, int32_t* out_indptr_a, int32_t* out_indices_a,
                                 int32_t* out_data_a, int32_t* out_indptr_n, int32_t* out_indices_n, int32_t* out_data_n, int32_t* out_row_line,
                                 uint64_t* out_sizes) {
    RCCHK(bus_check_args(records, n, bclen, umilen, flags, n_ecs, n_ec_targets, ec_ptr, ec_targets, n_targets, target_col, target_hap, n_loci, n_haps, keep,
                         n_keep, cap_cells, cap_rows, cap_a, cap_n, out_barcodes, out_indptr_a, out_indices_a, out_data_a, out_indptr_n, out_indices_n,
                         out_data_n, out_row_line, out_sizes));
    Call c(device, "bus: "); if (c.rc) return c.rc;
    DevBuf<> dr, dp, di, dc, dh, dk, ob, oipa, oixa, odaa, oipn, oixn, odn, orl;
    std::vector<StageIn> in = {{&dr, records, n * 32}, {&dp, ec_ptr, ((u64)n_ecs + 1) * 4}, {&di, ec_targets, n_ec_targets * 4},
                               {&dc, target_col, (u64)n_targets * 4}, {&dh, target_hap, (u64)n_targets * 4},
                               {&ob, nullptr, cap_cells * 8}, {&oipa, nullptr, (cap_rows + 1) * 4}, {&oixa, nullptr, cap_a * 4}, {&odaa, nullptr, cap_a * 4},
                               {&oipn, nullptr, (cap_cells + 1) * 4}, {&oixn, nullptr, cap_n * 4}, {&odn, nullptr, cap_n * 4}, {&orl, nullptr, cap_rows * 4}};
    if (keep) in.push_back({&dk, keep, n_keep * 8});
    int rc = stage_in(c, in);
    if (rc == ECB_OK)
        rc = ecb_bus_molecules_device(device, dr.p, n, bclen, umilen, flags, n_ecs, n_ec_targets, dp.p, di.p, n_targets, dc.p, dh.p, n_loci, n_haps,
                                      keep ? dk.p : nullptr, n_keep, cap_cells, cap_rows, cap_a, cap_n, ob.p, oipa.p, oixa.p, odaa.p, oipn.p, oixn.p, odn.p,
                                      orl.p, out_sizes);
    RCCHK(rc);
    const u64 cells = out_sizes[0], rows = out_sizes[1], nnz_a = out_sizes[2], nnz_n = out_sizes[3];
    return stage_out(c, {{out_barcodes, &ob, cells * 8}, {out_indptr_a, &oipa, (rows + 1) * 4}, {out_indices_a, &oixa, nnz_a * 4}, {out_data_a, &odaa, nnz_a * 4},
                         {out_indptr_n, &oipn, (cells + 1) * 4}, {out_indices_n, &oixn, nnz_n * 4}, {out_data_n, &odn, nnz_n * 4},
                         {out_row_line, &orl, rows * 4}});
}
