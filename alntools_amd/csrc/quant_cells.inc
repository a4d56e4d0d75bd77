// ---- ecquant per cell: one EM for every column of N, batched (ecb_cell_support* / ecb_quantify_cells*; included by ecb.hip) -----------------
// Cell c is a small problem of its own: its rows are the entries of column c of N with a count > 0 (an EC listed twice is two rows), its
// unknowns the (slot, h) of its support -- the loci its rows touch with a mask other than 0, ascending.  Many cells are iterated by the same
// launches: a BATCH is a stretch of cells in cell order whose expanded size (the row lengths of A summed over its entries of N) fits the
// budget and the sort's 2^30.  Set-up per batch: the row length of every entry (k_qc_len), a scan, one key (cell, locus) per expanded
// non-zero (k_qc_expand; a stored mask of 0 gets a key behind every cell and so leaves the support), one stable radix sort over the bits that
// vary, the runs of equal keys = the slots (k_qc_heads, a scan, k_qc_slots: slot pointers, the column view (entry, mask) per element, and
// through the sort's values the row view, the slot of every expanded non-zero), the cells' slot ranges and their chunks of TPB (slot, h)
// items (k_qc_cellptr, a scan, k_qc_chunks).  phi, theta and scale are cell-local, slots x H: what a cell gathers is its own few KB.
// One step, over the whole batch: E-step k_qc_estep (quant.inc's scheme: workgroup b stages the expanded non-zeros of entries
// [b TPB, (b + 1) TPB) through LDS, lane k adds those of entry k in index order; a workgroup whose cells are all done returns at once)
// and k_qc_elong (a workgroup per row longer than QC_LONG_ROW); M-step k_qc_mlong (a workgroup per column longer than QC_LONG_COL) and
// k_qc_mstep (workgroup q = chunk q of one cell: lane i one (slot, h), its column's entries in index order; the workgroup's |delta| folded
// by the tree); k_qc_conv (workgroup c = cell c: its chunks' parts in a fixed order, its explained reads, its step counted, its stop).
// No float atomics: every sum is one thread's in index order or one workgroup's strided partial sums folded by q_block_sum, and no sum
// spans two cells -- so a cell's bytes do not depend on which cells share its batch.  Converged cells are not compacted out: their
// workgroups return on the first load (measured share: profiles/ecquant_cells_c4.txt).  The per-cell reduce has one level: thread k of the
// cell's workgroup adds parts k, k + TPB, ... whatever their number.
// The validation front is quant.inc's q_front (every sample's counts as the weights); the E- and M-step kernels run quant.inc's bodies
// (q_tile_pass, q_long_row_sum, q_col_fold, q_theta_next) behind their own per-cell indexing and `done` tests.
namespace {
constexpr u32 QC_LONG_ROW = 256;     // an entry whose row has more non-zeros than this is summed by a workgroup, not a lane
constexpr u32 QC_LONG_COL = 32;      // a slot with more column entries than this likewise
constexpr u32 QC_TILE = 2048;        // k_qc_estep: expanded non-zeros of a workgroup's entries in LDS at a time
constexpr u32 QC_NONE = 0xFFFFFFFFu; // the slot of an expanded non-zero whose stored mask is 0
constexpr u64 QC_X_BYTES = 64;       // device bytes the set-up holds per expanded non-zero, besides ...
constexpr u64 QC_SLOT_TABLES = 4;    // ... this many slots x H x 8-byte tables (theta, phi, scale, the long columns' sums)
struct QcState { u32 n_long_rows, n_long_cols, running, pad; };

// the last k of [lo, hi] with ptr[k] <= i (ptr never falls)
template <class P> __device__ __forceinline__ u32 qc_last_le(const P* ptr, u32 lo, u32 hi, u64 i) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if ((u64)ptr[mid] <= i) lo = mid; else hi = mid - 1u;
    }
    return lo;
}
__device__ __forceinline__ bool qc_kept(const uint8_t* keep, u32 c) { return !keep || keep[c] != 0; }
// workgroup c: cell c's expanded size and W (its counts over the rows that hold a set bit), both exact; 0 for a cell that is not kept
__global__ __launch_bounds__(TPB) void k_qc_cells(const int* indptr_n, const int* indices_n, const int* data_n, const uint8_t* keep, const int* indptr_a,
                                                  const u32* bits_excl, u64* cell_x, u64* cell_w) {
    __shared__ u64 s[TPB];
    const u32 c = blockIdx.x;
    u64 x = 0, w = 0;
    if (qc_kept(keep, c))
        for (u32 j = (u32)indptr_n[c] + threadIdx.x, z = (u32)indptr_n[c + 1]; j < z; j += TPB) {
            const int n = data_n[j];
            if (n <= 0) continue;
            const u32 a = (u32)indptr_a[indices_n[j]], b = (u32)indptr_a[indices_n[j] + 1];
            x += b - a;
            if (bits_excl[b] != bits_excl[a]) w += (u64)n;
        }
    x = q_block_sum(x, s);
    __syncthreads();
    w = q_block_sum(w, s);
    if (threadIdx.x == 0) { cell_x[c] = x; cell_w[c] = w; }
}
// every cell: no slots, no step, converged -- what a cell that never runs reports
__global__ __launch_bounds__(TPB) void k_qc_info0(u32 n_cells, u32* cell_slots, u32* n_iter, double* delta, long long* explained, uint8_t* converged) {
    const u64 c = blockIdx.x * (u64)TPB + threadIdx.x;
    if (c >= n_cells) return;
    cell_slots[c] = 0u; n_iter[c] = 0u; delta[c] = 0.0; explained[c] = 0; converged[c] = 1;
}
// entry k of the batch (entry j0 + k of N): its cell within the batch, its row's length when it is a row of a kept cell (else 0: it
// expands to nothing), listed when it is long
__global__ __launch_bounds__(TPB) void k_qc_len(const int* indptr_n, const int* indices_n, const int* data_n, const uint8_t* keep, const int* indptr_a,
                                                u32 j0, u32 n_ent, u32 c0, u32 c1, u32* len, u32* ent_cell, QcState* st, u32* long_rows) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k >= n_ent) return;
    const u32 j = j0 + (u32)k, c = qc_last_le(indptr_n, c0, c1 - 1u, j);
    u32 n = 0;
    if (qc_kept(keep, c) && data_n[j] > 0) n = (u32)(indptr_a[indices_n[j] + 1] - indptr_a[indices_n[j]]);
    len[k] = n;
    ent_cell[k] = c - c0;
    if (n > QC_LONG_ROW) long_rows[atomicAdd(&st->n_long_rows, 1u)] = (u32)k;
}
// expanded non-zero x: its entry, its mask, its key (cell, locus) -- behind every cell when the stored mask is 0 -- and x as the value
__global__ __launch_bounds__(TPB) void k_qc_expand(const u32* off, u32 n_ent, u32 n_x, const u32* ent_cell, const int* indices_n, u32 j0,
                                                   const int* indptr_a, const int* indices_a, const int* data_a, u32 n_cells, u64* keys, u32* vals,
                                                   u32* x_ent, u32* x_mask) {
    const u64 x = blockIdx.x * (u64)TPB + threadIdx.x;
    if (x >= n_x) return;
    const u32 k = qc_last_le(off, 0u, n_ent - 1u, x);
    const u32 i = (u32)indptr_a[indices_n[j0 + k]] + ((u32)x - off[k]);
    const u32 m = (u32)data_a[i];
    keys[x] = m ? ((u64)ent_cell[k] << 32 | (u32)indices_a[i]) : ((u64)n_cells << 32);
    vals[x] = (u32)x;
    x_ent[x] = k;
    x_mask[x] = m;
}
// flag[i] = 1 where a slot starts: a run of equal sorted keys of a cell (the keys behind every cell start none)
__global__ __launch_bounds__(TPB) void k_qc_heads(const u64* keys, u32 n_x, u32 n_cells, u32* flag) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n_x) flag[i] = ((u32)(keys[i] >> 32) < n_cells && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}
// sorted element i: the column view (entry, mask), the row view through its value, and where its slot starts (pos = the exclusive scan of flag)
__global__ __launch_bounds__(TPB) void k_qc_slots(const u64* keys, const u32* vals, const u32* flag, const u32* pos, u32 n_x, u32 n_cells, const u32* x_ent,
                                                  const u32* x_mask, u32* row_slot, u32* col_ent, u32* col_mask, u32* slot_ptr, u32* slot_locus,
                                                  u32* slot_cell) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n_x) return;
    const u64 key = keys[i];
    const u32 x = vals[i];
    col_ent[i] = x_ent[x];
    col_mask[i] = x_mask[x];
    if ((u32)(key >> 32) >= n_cells) { row_slot[x] = QC_NONE; return; }
    const u32 s = pos[i] - (flag[i] ? 0u : 1u);
    row_slot[x] = s;
    if (flag[i]) { slot_ptr[s] = (u32)i; slot_locus[s] = (u32)key; slot_cell[s] = (u32)(key >> 32); }
    if (i + 1 == n_x || (u32)(keys[i + 1] >> 32) >= n_cells) slot_ptr[s + 1] = (u32)i + 1u;
}
// cell c of the batch (c <= n_cells): its first slot; its number of slots and of chunks
__global__ __launch_bounds__(TPB) void k_qc_cellptr(const u32* slot_cell, u32 n_slots, u32 n_cells, u32 n_haps, u32* cell_slot0, u32* cell_slots,
                                                    u32* n_chunks) {
    const u64 c = blockIdx.x * (u64)TPB + threadIdx.x;
    if (c > n_cells) return;
    u32 b[2];
    for (u32 k = 0; k < 2; ++k) {                  // the first slot whose cell is at or above c + k
        u32 lo = 0, hi = n_slots;
        while (lo < hi) { const u32 mid = (lo + hi) / 2u; if (slot_cell[mid] < c + k) lo = mid + 1u; else hi = mid; }
        b[k] = lo;
    }
    cell_slot0[c] = b[0];
    if (c < n_cells) { cell_slots[c] = b[1] - b[0]; n_chunks[c] = (u32)(((u64)(b[1] - b[0]) * n_haps + TPB - 1) / TPB); }
}
__global__ __launch_bounds__(TPB) void k_qc_chunks(const u32* chunk_ptr, u32 n_cells, u32 n_chunks, u32* chunk_cell) {
    const u64 q = blockIdx.x * (u64)TPB + threadIdx.x;
    if (q < n_chunks) chunk_cell[q] = qc_last_le(chunk_ptr, 0u, n_cells - 1u, q);
}
__global__ __launch_bounds__(TPB) void k_qc_cols(const u32* slot_ptr, u32 n_slots, QcState* st, u32* long_cols) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s < n_slots && slot_ptr[s + 1] - slot_ptr[s] > QC_LONG_COL) long_cols[atomicAdd(&st->n_long_cols, 1u)] = (u32)s;
}
// cell c of the batch: its stop; done from the start when it has no slot or no step is asked for, else counted as running
__global__ __launch_bounds__(TPB) void k_qc_arm(const u32* cell_slots, const u64* cell_w, u32 n_cells, u32 max_iters, double tol, double* stop, u32* done,
                                                QcState* st) {
    const u64 c = blockIdx.x * (u64)TPB + threadIdx.x;
    if (c >= n_cells) return;
    stop[c] = tol * (double)cell_w[c];
    const u32 d = cell_slots[c] == 0u || max_iters == 0u;
    done[c] = d;
    if (!d) atomicAdd(&st->running, 1u);
}
// item i = slot x H + h: the shared tables (T x H) brought to the slots; theta_0 = theta_in when there is one
__global__ __launch_bounds__(TPB) void k_qc_tabs(const u32* slot_locus, u64 n_items, u32 n_haps, const double* tab_scale, const double* tab_theta,
                                                 double* scale, double* theta, double* phi) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n_items) return;
    const u32 s = (u32)(i / n_haps), h = (u32)(i - (u64)s * n_haps);
    const u64 g = (u64)slot_locus[s] * n_haps + h;
    if (tab_scale) scale[i] = tab_scale[g];
    if (tab_theta) { const double v = tab_theta[g]; theta[i] = v; phi[i] = tab_scale ? v * tab_scale[g] : v; }
}
// E-step, the short rows: k_q_estep's scheme over the batch's entries (off = the entries' places in the expansion, row_slot / x_mask the
// slot and mask of every expanded non-zero).  An entry of a cell that is done is nobody's; a workgroup of such entries returns at once.
// expl[k] = 1 when entry k's reads were explained (d > 0)
__global__ __launch_bounds__(TPB) void k_qc_estep(const u32* done, const u32* ent_cell, const u32* off, u32 n_ent, const u32* row_slot, const u32* x_mask,
                                                  const int* data_n, u32 j0, const double* phi, u32 n_haps, double* r, uint8_t* expl) {
    __shared__ double v[QC_TILE];
    const u64 k0 = blockIdx.x * (u64)TPB, k = k0 + threadIdx.x;
    u32 a = 0, b = 0;
    bool mine = false;
    if (k < n_ent) { a = off[k]; b = off[k + 1]; mine = b > a && b - a <= QC_LONG_ROW && !done[ent_cell[k]]; }
    if (!__syncthreads_or(mine)) return;
    const u32 lo = off[k0], hi = off[std::min<u64>(n_ent, k0 + TPB)];
    const double d = q_tile_pass<QC_TILE>(v, phi, n_haps, row_slot, x_mask, lo, hi, a, b, mine);
    if (mine) {
        u64 got;
        q_row_done((u64)data_n[j0 + k], d, r + k, got);
        expl[k] = got != 0;
    }
}
// E-step, workgroup b: long entry long_rows[b] -- thread k sums its non-zeros k, k + TPB, ... in that order, the tree folds the TPB sums
__global__ __launch_bounds__(TPB) void k_qc_elong(const u32* done, const u32* ent_cell, const u32* long_rows, const u32* off, const u32* row_slot,
                                                  const u32* x_mask, const int* data_n, u32 j0, const double* phi, u32 n_haps, double* r, uint8_t* expl) {
    __shared__ double s[TPB];
    const u32 k = long_rows[blockIdx.x];
    if (done[ent_cell[k]]) return;
    const double d = q_long_row_sum(s, phi, n_haps, row_slot, x_mask, off[k], off[k + 1]);
    if (threadIdx.x == 0) {
        u64 got;
        q_row_done((u64)data_n[j0 + k], d, r + k, got);
        expl[k] = got != 0;
    }
}
// M-step, workgroup b: long column long_cols[b] (a slot), k_q_mlong's scheme: q_col_fold over its entries' r.
// INIT: the sums of the counts instead (theta_0 = the cell's alignment counts), exact in 64-bit integers
template <bool INIT>
__global__ __launch_bounds__(TPB) void k_qc_mlong(const u32* done, const u32* slot_cell, const u32* long_cols, const u32* slot_ptr, const u32* col_ent,
                                                  const u32* col_mask, const double* r, const int* data_n, u32 j0, u32 n_haps, u32 hp, double* acc_long) {
    using V = typename std::conditional<INIT, u64, double>::type;
    __shared__ V s[TPB], val[TPB];
    __shared__ u32 msk[TPB];
    const u32 t = long_cols[blockIdx.x];
    if (!INIT && done[slot_cell[t]]) return;
    const V acc = q_col_fold(s, val, msk, col_mask, slot_ptr[t], slot_ptr[t + 1], hp,
                             [&](u32 k) { if constexpr (INIT) return (V)data_n[j0 + col_ent[k]]; else return (V)r[col_ent[k]]; }, [](V x, u32, u32) { return x; });
    if (threadIdx.x < n_haps) acc_long[(u64)t * n_haps + threadIdx.x] = (double)acc;
}
// M-step, workgroup q: chunk q of one cell; lane i one (slot, h) of it: the entries of the slot's column with bit h, in index order (entry
// order); theta', the next phi, and the chunk's part of the cell's delta.  INIT: theta_0 = the cell's alignment counts, no delta
template <bool INIT>
__global__ __launch_bounds__(TPB) void k_qc_mstep(const u32* done, const u32* chunk_cell, const u32* chunk_ptr, const u32* cell_slot0, const u32* slot_ptr,
                                                  const u32* col_ent, const u32* col_mask, const double* r, const int* data_n, u32 j0,
                                                  const double* acc_long, const double* scale, u32 n_haps, double* theta, double* phi, double* partial) {
    __shared__ double s[TPB];
    const u32 c = chunk_cell[blockIdx.x];
    if (!INIT && done[c]) return;
    const u64 item = (u64)(blockIdx.x - chunk_ptr[c]) * TPB + threadIdx.x;
    const u64 i = (u64)cell_slot0[c] * n_haps + item;
    double diff = 0.0;
    if (item < (u64)(cell_slot0[c + 1] - cell_slot0[c]) * n_haps) {
        const u32 t = (u32)(i / n_haps), h = (u32)(i - (u64)t * n_haps);
        const u32 a = slot_ptr[t], b = slot_ptr[t + 1];
        double acc;
        if (b - a > QC_LONG_COL) acc = acc_long[i];
        else if (INIT) {
            u64 n = 0;
            for (u32 k = a; k < b; ++k)
                if ((col_mask[k] >> h) & 1u) n += (u64)data_n[j0 + col_ent[k]];
            acc = (double)n;
        } else {
            acc = 0.0;
            for (u32 k = a; k < b; ++k)
                if ((col_mask[k] >> h) & 1u) acc += r[col_ent[k]];
        }
        diff = q_theta_next<INIT>(acc, i, scale, theta, phi);
    }
    if (INIT) return;
    diff = q_block_sum(diff, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = diff;
}
// workgroup c: cell c of the batch (c0 + c of the call) -- delta = its chunks' parts in a fixed order (thread k: parts k, k + TPB, ...; then
// the tree), the explained reads over its entries likewise (integers); its step counted, its stop decided
__global__ __launch_bounds__(TPB) void k_qc_conv(u32* done, const u32* chunk_ptr, const double* partial, const int* indptr_n, const int* data_n, u32 j0,
                                                 u32 c0, const uint8_t* expl, const u32* len, const double* stop, u32 max_iters, QcState* st, u32* n_iter,
                                                 double* delta, long long* explained, uint8_t* converged) {
    __shared__ double s[TPB];
    __shared__ u64 sw[TPB];
    const u32 c = blockIdx.x;
    if (done[c]) return;
    u64 got = 0;
    for (u32 j = (u32)indptr_n[c0 + c] + threadIdx.x, z = (u32)indptr_n[c0 + c + 1]; j < z; j += TPB)
        if (len[j - j0] && expl[j - j0]) got += (u64)data_n[j];
    got = q_block_sum(got, sw);
    double d = 0.0;
    for (u32 k = chunk_ptr[c] + threadIdx.x, z = chunk_ptr[c + 1]; k < z; k += TPB) d += partial[k];
    d = q_block_sum(d, s);
    if (threadIdx.x != 0) return;
    const u32 n = n_iter[c0 + c] + 1u;
    n_iter[c0 + c] = n;
    delta[c0 + c] = d;
    explained[c0 + c] = (long long)got;
    const bool conv = d <= stop[c];
    converged[c0 + c] = conv;
    if (conv || n >= max_iters) { done[c] = 1u; atomicSub(&st->running, 1u); }
}

// a batch's own device buffers: freed when the batch ends, but for those taken out for the call's end
struct QcBufs {
    std::vector<DevBuf<>> v;
    bool short_of = false;
    template <class T> T* get(u64 n) {
        v.emplace_back();
        short_of |= v.back().alloc(std::max<u64>(n, 1) * sizeof(T)) != hipSuccess;
        return v.back().as<T>();
    }
};
struct QcKept { DevBuf<> locus, theta; u64 slot0, n_slots; };      // a batch's results until the whole support is known

// The hierarchical models per cell (ecb_quantify_cells_model*, quant_cells_model.inc, included after this file) run on a batch as qc_run
// set it up: what it hands them (QcView), what they add to the set-up (QcmTabs, the batch's buffers) and their step in place of the E- and
// M-step kernels.  mdl = nullptr: the flat step, this file's own.
struct QcView {
    hipStream_t st;
    u32 j0, n_ent, nc, n_x, n_slots, n_haps, hp, nlr, nlc, nq;
    const int* data_n;
    const u32 *done, *ent_cell, *off, *long_rows, *x_ent, *x_mask, *row_slot, *col_mask, *slot_ptr, *slot_locus, *slot_cell, *long_cols, *cell_slot0,
        *chunk_cell, *chunk_ptr;
    u32 *flag, *pos;                 // free once the slots stand: the set-up's scans
    const double* scale;
    double *theta, *phi, *acc_long, *partial;
    uint8_t* expl;
};
struct QcmTabs {
    u32 n_groups, n_segs, n_long_groups;
    u32 *slot_group, *gptr, *gmem, *group_cell, *long_groups;          // the (cell, gene) groups: every slot's, and their members as a CSR
    u32 *segid, *seg_start, *seg_group, *seg_cell, *gx, *x_seg;        // the (entry, group) segments of the rows, over the gene-ordered view
    u32 *x_b0, *col_b0;                                                // where the coefficients of a non-zero start: row view, column view
    double *phi_gh, *phi_g, *phi_t, *seg_c, *seg_x, *coef;
};
u64 qcm_x_bytes(u32 n_haps);
int qcm_setup(Call& c, QcBufs& q, const QcView& v, const QModel& mdl, SortBufs& s, const SortScratch& ss, u32* sums, QcmTabs& t);
void qcm_step(const QcView& v, const QcmTabs& t, u32 model);

int qc_check_args(const QMat& m, const char* what) {
    // (no sample is no refusal here: there is then nothing to quantify)
    RCCHK(ca_check_matrices(m.n_ecs, m.n_loci, m.n_haps, m.nnz, m.ip, m.ix, m.da, std::max<uint32_t>(m.n_samples, 1u), m.nnz_n, m.pn, m.xn, m.dn));
    if (m.nnz >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "%s: 2^30 non-zeros or more", what);
    if ((u64)m.n_haps * m.n_loci >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "%s: haplotypes x loci does not fit 31 bits", what);
    return ECB_OK;
}
// ... and what the four ecquant-cells entry points refuse after that
int qc_check_quant(const QMat& m, const void* cell_ptr, const void* slot_locus, const void* theta, uint64_t n_slots, double tol) {
    RCCHK(qc_check_args(m, "ecquant-cells"));
    if (!cell_ptr || (n_slots && (!slot_locus || !theta)) || !(tol >= 0.0))          // (an array of no slots may be null)
        return fail(nullptr, ECB_ERR_ARG, "ecquant-cells: bad argument (no cell_ptr, slot_locus or theta, or a tolerance that is NaN or negative)");
    if (n_slots >= (1ull << 31) || n_slots * m.n_haps >= (1ull << 32))
        return fail(nullptr, ECB_ERR_LIMIT, "ecquant-cells: n_slots is %llu: 2^31 slots or 2^32 values of theta, or more", (unsigned long long)n_slots);
    return ECB_OK;
}

// what a run writes for the caller (device memory; those from n_iter on may be null)
struct QcOut { void *cell_ptr, *slot_locus, *theta, *n_iter, *delta, *explained, *converged; };
// All device entry points, their arguments checked.  quant = false: the support alone (of `o` only cell_ptr and slot_locus are used; n_slots_in =
// the capacity of o.slot_locus).  mdl = nullptr: the flat step; model 4 is that step too, the genes checked first in a call of their own.
int qc_run(bool quant, int device, const QMat& m, const void* d_cell_keep, const void* d_scale, const void* d_theta_in, u32 max_iters, double tol,
           u64 budget_bytes, u64 n_slots_in, const QcOut& o, uint64_t* n_slots_out, const QModel* mdl = nullptr) {
    if (mdl && mdl->model == 4u) {
        RCCHK(qm_check_genes(device, "ecquant-cells: ", mdl->gene, m.n_loci, mdl->n_genes));
        mdl = nullptr;
    }
    const char* what = quant ? "ecquant-cells" : "cell-support";
    Call c(device, quant ? "ecquant-cells: " : "cell-support: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u32 S = m.n_samples, n_loci = m.n_loci, n_haps = m.n_haps;
    const u64 nnz = m.nnz;
    // the front, every sample's counts as the weights (which only its check of N needs); words [6] [7]: a batch's totals
    QFront f;
    RCCHK(q_front(c, m, -1, quant ? d_scale : nullptr, quant ? d_theta_in : nullptr, Q_ERR_THETA, false, mdl ? mdl->gene : nullptr, mdl ? mdl->n_genes : 0u,
                  false, nnz, Q_ERRS, f));
    u64* words = f.words;
    u32 *bits_excl = f.bits_excl, *sums = f.sums;
    double *tab_scale = f.scale, *tab_theta = f.theta;
    u64 *cell_x = c.get<u64>(S), *cell_w = c.get<u64>(S);
    u32 *cell_slots = c.get<u32>(S), *it = c.get<u32>(S);
    double* dl = c.get<double>(S);
    long long* ex = c.get<long long>(S);
    uint8_t* cv = c.get<uint8_t>(S);
    if (const int rc = c.missing()) return rc;
    const int *ip = m.ip, *ix = m.ix, *da = m.da, *pn = m.pn, *xn = m.xn, *dn = m.dn;
    const uint8_t* keep = (const uint8_t*)d_cell_keep;
    // the input is well formed.  The cells' sizes, and from them the batches
    std::vector<u64> hx(S);
    if (S) {
        k_qc_cells<<<S, TPB, 0, st>>>(pn, xn, dn, keep, ip, bits_excl, cell_x, cell_w);
        k_qc_info0<<<nblk(S, TPB), TPB, 0, st>>>(S, cell_slots, it, dl, ex, cv);
        CALLCHK(c, hipGetLastError());
        if (const int rc = c.read_back(hx.data(), cell_x, S)) return rc;
    }
    for (u32 k = 0; k < S; ++k)
        if (hx[k] >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "%s: cell %u alone expands to 2^30 non-zeros or more", what, k);
    std::vector<int> hpn((u64)S + 1, 0);
    if (S) { CALLCHK(c, hipMemcpyAsync(hpn.data(), pn, ((u64)S + 1) * 4, hipMemcpyDeviceToHost, st)); CALLCHK(c, hipStreamSynchronize(st)); }
    if (!budget_bytes) {                               // half of what is free now (a target: a cell that alone exceeds it still runs, alone)
        size_t fr = 0, tot = 0;
        CALLCHK(c, hipMemGetInfo(&fr, &tot));
        budget_bytes = std::max<u64>(fr / 2, 1);
    }
    u64 x_limit = std::min<u64>((1ull << 30) - 1, std::max<u64>(1, budget_bytes / (QC_X_BYTES + QC_SLOT_TABLES * 8 * n_haps + (mdl ? qcm_x_bytes(n_haps) : 0))));
    if (mdl) x_limit = std::min<u64>(x_limit, ((1ull << 32) - 1) / std::max<u32>(n_haps, 1u));          // (a batch's coefficients, one per set bit, are indexed in 32 bits)
    struct Batch { u32 c0, c1; u64 x; };
    std::vector<Batch> batches;
    u64 max_x = 0, max_ent = 0, max_cells = 0;
    for (u32 k = 0; k < S;) {
        Batch b{k, k, 0};
        while (b.c1 < S && (b.x == 0 || b.x + hx[b.c1] <= x_limit)) b.x += hx[b.c1++];
        k = b.c1;
        if (!b.x) continue;                            // (cells that expand to nothing: no slots, as k_qc_info0 left them)
        batches.push_back(b);
        max_x = std::max(max_x, b.x); max_ent = std::max<u64>(max_ent, (u64)(hpn[b.c1] - hpn[b.c0])); max_cells = std::max<u64>(max_cells, b.c1 - b.c0);
    }
    u64 *k0 = nullptr, *k1 = nullptr; u32 *v0 = nullptr, *v1 = nullptr;
    SortScratch ss{};
    if (!batches.empty()) {
        k0 = c.get<u64>(CV_KEYS0, max_x); k1 = c.get<u64>(CV_KEYS1, max_x); v0 = c.get<u32>(CV_VALS0, max_x); v1 = c.get<u32>(CV_VALS1, max_x);
        ss = SortScratch{c.get<u32>(CV_HIST, rs_words(max_x)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 4};
        sums = c.get<u32>(CV_SUMS2, scan_words(std::max(std::max(max_x, max_ent), std::max<u64>(max_cells, nnz))));
        if (const int rc = c.missing()) return rc;
    }
    u32 hp = 1;
    while (hp < n_haps) hp <<= 1;
    std::vector<QcKept> kept;
    u64 total_slots = 0;
    for (const Batch& b : batches) {
        const u32 j0 = (u32)hpn[b.c0], n_ent = (u32)(hpn[b.c1] - hpn[b.c0]), nc = b.c1 - b.c0, n_x = (u32)b.x;
        QcBufs q;
        QcState* qs = q.get<QcState>(1);
        u32 *len = q.get<u32>(n_ent), *off = q.get<u32>((u64)n_ent + 1), *ent_cell = q.get<u32>(n_ent), *long_rows = q.get<u32>(n_x / QC_LONG_ROW + 1);
        u32 *x_ent = q.get<u32>(n_x), *x_mask = q.get<u32>(n_x), *flag = q.get<u32>(n_x), *pos = q.get<u32>(n_x);
        u32 *row_slot = q.get<u32>(n_x), *col_ent = q.get<u32>(n_x), *col_mask = q.get<u32>(n_x);
        u32 *cell_slot0 = q.get<u32>((u64)nc + 1), *n_chunks = q.get<u32>(nc), *chunk_ptr = q.get<u32>((u64)nc + 1), *done = q.get<u32>(nc);
        double* stop = q.get<double>(nc);
        if (q.short_of) return fail(nullptr, ECB_ERR_HIP, "%sout of device memory", c.prefix);
        CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QcState), st));
        k_qc_len<<<nblk(n_ent, TPB), TPB, 0, st>>>(pn, xn, dn, keep, ip, j0, n_ent, b.c0, b.c1, len, ent_cell, qs, long_rows);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, scan_launch(st, len, n_ent, off, sums, nullptr, 1, off + n_ent));
        k_qc_expand<<<nblk(n_x, TPB), TPB, 0, st>>>(off, n_ent, n_x, ent_cell, xn, j0, ip, ix, da, nc, k0, v0, x_ent, x_mask);
        CALLCHK(c, hipGetLastError());
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, n_x, ss, msb_mask(nc) << 32 | msb_mask(n_loci - 1)));
        k_qc_heads<<<nblk(n_x, TPB), TPB, 0, st>>>(s.keys(), n_x, nc, flag);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, scan_launch(st, flag, n_x, pos, sums, words + 6));
        u64 ns64 = 0;
        if (const int rc = c.read_back(&ns64, words + 6, 1)) return rc;
        const u32 n_slots = (u32)ns64;
        if (!n_slots) continue;                        // (only stored masks of 0)
        const u64 n_items = (u64)n_slots * n_haps;
        QcKept out;
        CALLCHK(c, out.locus.alloc((u64)n_slots * 4));
        u32 *slot_locus = out.locus.as<u32>(), *slot_ptr = q.get<u32>((u64)n_slots + 1), *slot_cell = q.get<u32>(n_slots);
        u32* long_cols = q.get<u32>(n_x / QC_LONG_COL + 1);
        if (q.short_of) return fail(nullptr, ECB_ERR_HIP, "%sout of device memory", c.prefix);
        k_qc_slots<<<nblk(n_x, TPB), TPB, 0, st>>>(s.keys(), s.vals(), flag, pos, n_x, nc, x_ent, x_mask, row_slot, col_ent, col_mask, slot_ptr, slot_locus,
                                                   slot_cell);
        k_qc_cellptr<<<nblk((u64)nc + 1, TPB), TPB, 0, st>>>(slot_cell, n_slots, nc, n_haps, cell_slot0, cell_slots + b.c0, n_chunks);
        CALLCHK(c, hipGetLastError());
        out.slot0 = total_slots; out.n_slots = n_slots;
        total_slots += n_slots;
        if (quant) {
            CALLCHK(c, scan_launch(st, n_chunks, nc, chunk_ptr, sums, words + 7, 1, chunk_ptr + nc));
            k_qc_cols<<<nblk(n_slots, TPB), TPB, 0, st>>>(slot_ptr, n_slots, qs, long_cols);
            k_qc_arm<<<nblk(nc, TPB), TPB, 0, st>>>(cell_slots + b.c0, cell_w + b.c0, nc, max_iters, tol, stop, done, qs);
            CALLCHK(c, hipGetLastError());
            QcState q0;
            u64 nq64 = 0;
            CALLCHK(c, hipMemcpyAsync(&q0, qs, sizeof(QcState), hipMemcpyDeviceToHost, st));
            if (const int rc = c.read_back(&nq64, words + 7, 1)) return rc;
            const u32 nlr = q0.n_long_rows, nlc = q0.n_long_cols, nq = (u32)nq64, n_eblk = nblk(n_ent, TPB);
            CALLCHK(c, out.theta.alloc(n_items * 8));
            double *theta = out.theta.as<double>(), *phi = q.get<double>(n_items), *scale = tab_scale ? q.get<double>(n_items) : nullptr;
            double *acc_long = q.get<double>(nlc ? n_items : 1), *partial = q.get<double>(nq), *r = q.get<double>(n_ent);
            u32* chunk_cell = q.get<u32>(nq);
            uint8_t* expl = q.get<uint8_t>(n_ent);
            if (q.short_of) return fail(nullptr, ECB_ERR_HIP, "%sout of device memory", c.prefix);
            const QcView view{st, j0, n_ent, nc, n_x, n_slots, n_haps, hp, nlr, nlc, nq, dn, done, ent_cell, off, long_rows, x_ent, x_mask, row_slot, col_mask,
                              slot_ptr, slot_locus, slot_cell, long_cols, cell_slot0, chunk_cell, chunk_ptr, flag, pos, scale, theta, phi, acc_long, partial, expl};
            QcmTabs mt{};
            if (mdl) RCCHK(qcm_setup(c, q, view, *mdl, s, ss, sums, mt));          // (before anything else sorts: it reads the column view's order)
            k_qc_chunks<<<nblk(nq, TPB), TPB, 0, st>>>(chunk_ptr, nc, nq, chunk_cell);
            if (tab_scale || tab_theta) k_qc_tabs<<<nblk(n_items, TPB), TPB, 0, st>>>(slot_locus, n_items, n_haps, tab_scale, tab_theta, scale, theta, phi);
            if (!tab_theta) {
                if (nlc) k_qc_mlong<true><<<nlc, TPB, 0, st>>>(done, slot_cell, long_cols, slot_ptr, col_ent, col_mask, r, dn, j0, n_haps, hp, acc_long);
                k_qc_mstep<true><<<nq, TPB, 0, st>>>(done, chunk_cell, chunk_ptr, cell_slot0, slot_ptr, col_ent, col_mask, r, dn, j0, acc_long, scale, n_haps,
                                                     theta, phi, partial);
            }
            CALLCHK(c, hipGetLastError());
            u32 running = q0.running;
            for (u32 queued = 0; running && queued < max_iters;) {
                for (u32 k = 0; k < Q_BATCH && queued < max_iters; ++k, ++queued) {
                    if (mdl) qcm_step(view, mt, mdl->model);
                    else {
                        if (nlr) k_qc_elong<<<nlr, TPB, 0, st>>>(done, ent_cell, long_rows, off, row_slot, x_mask, dn, j0, phi, n_haps, r, expl);
                        k_qc_estep<<<n_eblk, TPB, 0, st>>>(done, ent_cell, off, n_ent, row_slot, x_mask, dn, j0, phi, n_haps, r, expl);
                        if (nlc) k_qc_mlong<false><<<nlc, TPB, 0, st>>>(done, slot_cell, long_cols, slot_ptr, col_ent, col_mask, r, dn, j0, n_haps, hp, acc_long);
                        k_qc_mstep<false><<<nq, TPB, 0, st>>>(done, chunk_cell, chunk_ptr, cell_slot0, slot_ptr, col_ent, col_mask, r, dn, j0, acc_long, scale,
                                                              n_haps, theta, phi, partial);
                    }
                    k_qc_conv<<<nc, TPB, 0, st>>>(done, chunk_ptr, partial, pn, dn, j0, b.c0, expl, len, stop, max_iters, qs, it, dl, ex, cv);
                }
                CALLCHK(c, hipGetLastError());
                CALLCHK(c, hipMemcpyAsync(&q0, qs, sizeof(QcState), hipMemcpyDeviceToHost, st));
                CALLCHK(c, hipStreamSynchronize(st));
                running = q0.running;
            }
        }
        CALLCHK(c, hipStreamSynchronize(st));          // (the batch's buffers go here)
        kept.push_back(std::move(out));
    }
    if (total_slots >= (1ull << 31) || total_slots * n_haps >= (1ull << 32))
        return fail(nullptr, ECB_ERR_LIMIT, "%s: the support has %llu slots: 2^31 slots or 2^32 values of theta, or more", what, (unsigned long long)total_slots);
    if (quant && total_slots != n_slots_in)
        return fail(nullptr, ECB_ERR_ARG, "ecquant-cells: n_slots is %llu, the support has %llu slots", (unsigned long long)n_slots_in,
                    (unsigned long long)total_slots);
    // the whole support is known: from here on the outputs are written
    std::vector<u32> hs(S);
    std::vector<u64> hcum((u64)S + 1, 0);
    if (S) {
        CALLCHK(c, hipMemcpyAsync(hs.data(), cell_slots, (u64)S * 4, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
    }
    for (u32 k = 0; k < S; ++k) hcum[k + 1] = hcum[k] + hs[k];
    CALLCHK(c, hipMemcpyAsync(o.cell_ptr, hcum.data(), ((u64)S + 1) * 8, hipMemcpyHostToDevice, st));      // (int64, never negative)
    if (o.slot_locus && (quant || n_slots_in >= total_slots))
        for (const QcKept& k : kept) CALLCHK(c, hipMemcpyAsync((u32*)o.slot_locus + k.slot0, k.locus.p, k.n_slots * 4, hipMemcpyDeviceToDevice, st));
    if (quant) {
        for (const QcKept& k : kept)
            CALLCHK(c, hipMemcpyAsync((double*)o.theta + k.slot0 * n_haps, k.theta.p, k.n_slots * n_haps * 8, hipMemcpyDeviceToDevice, st));
        if (S && o.n_iter) CALLCHK(c, hipMemcpyAsync(o.n_iter, it, (u64)S * 4, hipMemcpyDeviceToDevice, st));
        if (S && o.delta) CALLCHK(c, hipMemcpyAsync(o.delta, dl, (u64)S * 8, hipMemcpyDeviceToDevice, st));
        if (S && o.explained) CALLCHK(c, hipMemcpyAsync(o.explained, ex, (u64)S * 8, hipMemcpyDeviceToDevice, st));
        if (S && o.converged) CALLCHK(c, hipMemcpyAsync(o.converged, cv, (u64)S, hipMemcpyDeviceToDevice, st));
    }
    CALLCHK(c, hipStreamSynchronize(st));
    if (n_slots_out) *n_slots_out = total_slots;
    return ECB_OK;
}
// Both host entry points of ecquant-cells, their arguments checked: everything staged, the device run, the results back
int qc_host(int device, const QMat& m, const uint8_t* cell_keep, const double* scale, const double* theta_in, u32 max_iters, double tol, u64 budget_bytes,
            const QModel* mdl, u64 n_slots, int64_t* cell_ptr, int32_t* slot_locus, double* theta, uint32_t* n_iter, double* delta, int64_t* explained,
            uint8_t* converged) {
    Call c(device, "ecquant-cells: "); if (c.rc) return c.rc;
    const u64 plane = (u64)m.n_haps * m.n_loci * 8, S = m.n_samples;
    QStage b;
    DevBuf<> kp, sc, ti, gn, ocp, osl, oth, oit, odl, oex, ocv;
    std::vector<StageIn> in = q_stage(b, m);
    if (mdl) in.push_back({&gn, mdl->gene, (u64)m.n_loci * 4});
    in.insert(in.end(), {{&ocp, nullptr, (S + 1) * 8}, {&osl, nullptr, n_slots * 4}, {&oth, nullptr, n_slots * m.n_haps * 8},
                         {&oit, nullptr, S * 4}, {&odl, nullptr, S * 8}, {&oex, nullptr, S * 8}, {&ocv, nullptr, S}});
    if (cell_keep) in.push_back({&kp, cell_keep, S});
    if (scale) in.push_back({&sc, scale, plane});
    if (theta_in) in.push_back({&ti, theta_in, plane});
    RCCHK(stage_in(c, in));
    const QModel dm{mdl ? mdl->model : 4u, mdl ? mdl->n_genes : 0u, gn.as<int>()};
    RCCHK(qc_run(true, device, q_staged(b, m), kp.p, sc.p, ti.p, max_iters, tol, budget_bytes, n_slots, QcOut{ocp.p, osl.p, oth.p, oit.p, odl.p, oex.p, ocv.p},
                 nullptr, mdl ? &dm : nullptr));
    return stage_out(c, {{cell_ptr, &ocp, (S + 1) * 8}, {slot_locus, &osl, n_slots * 4}, {theta, &oth, n_slots * m.n_haps * 8},
                         {n_iter, &oit, n_iter ? S * 4 : 0}, {delta, &odl, delta ? S * 8 : 0}, {explained, &oex, explained ? S * 8 : 0},
                         {converged, &ocv, converged ? S : 0}});
}
}  // namespace

extern "C" int ecb_cell_support_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                       const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                       const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, void* d_cell_ptr, void* d_slot_locus,
                                       uint64_t slot_capacity, uint64_t* n_slots) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(qc_check_args(m, "cell-support"));
    if (!d_cell_ptr) return fail(nullptr, ECB_ERR_ARG, "cell-support: bad argument (no cell_ptr)");
    return qc_run(false, device, m, d_cell_keep, nullptr, nullptr, 0, 0.0, 0, slot_capacity, QcOut{d_cell_ptr, d_slot_locus}, n_slots);
}

extern "C" int ecb_cell_support(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                                const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, int64_t* cell_ptr, int32_t* slot_locus,
                                uint64_t slot_capacity, uint64_t* n_slots) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(qc_check_args(m, "cell-support"));
    if (!cell_ptr) return fail(nullptr, ECB_ERR_ARG, "cell-support: bad argument (no cell_ptr)");
    Call c(device, "cell-support: "); if (c.rc) return c.rc;
    QStage b;
    DevBuf<> kp, ocp, osl;
    std::vector<StageIn> in = q_stage(b, m);
    in.push_back({&ocp, nullptr, ((u64)n_samples + 1) * 8});
    if (cell_keep) in.push_back({&kp, cell_keep, n_samples});
    if (slot_locus && slot_capacity) in.push_back({&osl, nullptr, slot_capacity * 4});
    RCCHK(stage_in(c, in));
    uint64_t ns = 0;
    RCCHK(qc_run(false, device, q_staged(b, m), kp.p, nullptr, nullptr, 0, 0.0, 0, osl.p ? slot_capacity : 0, QcOut{ocp.p, osl.p}, &ns));
    RCCHK(stage_out(c, {{cell_ptr, &ocp, ((u64)n_samples + 1) * 8}, {slot_locus, &osl, osl.p && slot_capacity >= ns ? ns * 4 : 0}}));
    if (n_slots) *n_slots = ns;
    return ECB_OK;
}

extern "C" int ecb_quantify_cells_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                         const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                         const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, const void* d_scale,
                                         const void* d_theta_in, uint32_t max_iters, double tol, uint64_t budget_bytes, uint64_t n_slots,
                                         void* d_cell_ptr, void* d_slot_locus, void* d_theta, void* d_n_iter, void* d_delta, void* d_explained,
                                         void* d_converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(qc_check_quant(m, d_cell_ptr, d_slot_locus, d_theta, n_slots, tol));
    return qc_run(true, device, m, d_cell_keep, d_scale, d_theta_in, max_iters, tol, budget_bytes, n_slots,
                  QcOut{d_cell_ptr, d_slot_locus, d_theta, d_n_iter, d_delta, d_explained, d_converged}, nullptr);
}

extern "C" int ecb_quantify_cells(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                                  const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                  const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, const double* scale, const double* theta_in,
                                  uint32_t max_iters, double tol, uint64_t budget_bytes, uint64_t n_slots, int64_t* cell_ptr, int32_t* slot_locus,
                                  double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint8_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(qc_check_quant(m, cell_ptr, slot_locus, theta, n_slots, tol));
    return qc_host(device, m, cell_keep, scale, theta_in, max_iters, tol, budget_bytes, nullptr, n_slots, cell_ptr, slot_locus, theta, n_iter, delta,
                   explained, converged);
}
