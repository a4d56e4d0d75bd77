// ---- ecquant per cell with EMASE's hierarchical models (ecb_quantify_cells_model / ecb_quantify_cells_model_device; included by ecb.hip after
// quant_cells.inc) ------------------------------------------------------------------------------------------------------------------------
// A batch of cells is one block-diagonal problem in slot coordinates: rows = the batch's entries, columns = its slots, groups = the distinct
// (cell, gene[slot_locus]) pairs.  quant_model.inc's step on that problem, with groups that never cross a cell, is the model of every cell
// alone: Phi_gh, Phi_g and Phi_t are sums over the cell's support only.  Only the stop is per cell (k_qc_conv, unchanged).
// Set-up per batch, after qc_run's (qcm_setup): the set bits of every expanded non-zero counted and scanned = where its coefficients start,
// brought to the column view through the first sort's values; the slots sorted on (cell, gene), stable -- a cell's slots ascend by locus, so
// a group's members are scattered over the cell's range and come together only here, loci still ascending --, run heads and a scan = each
// slot's group and each group's members as a CSR; the expanded non-zeros sorted on (entry, group), stable = the gene-ordered view of the rows,
// its run heads and a scan = the segments (an expanded non-zero with a stored mask of 0 has no slot: its key is behind every group, its
// segment never alive).
// One step (qcm_step), every kernel leaving a finished cell's work on the first load:
//   k_qcm_gh [k_qcm_ghlong]    Phi_gh per group (a group with more than Q_LONG_GENE members: a workgroup)
//   k_qcm_g                    Phi_g per group; model 2: Phi_t per slot
//   k_qcm_seg / k_qcm_seg1     per segment: alive or not, and its divisor (quant_model.inc's definitions)
//   [k_qcm_rowlong] k_qcm_row  per entry: the gene denominator, w over it, explained or not (k_qc_conv adds the counts); its segments' c
//   k_qcm_coef                 one coefficient per set bit, in the expansion's order
//   [k_qcm_mlong] k_qcm_mstep  theta' = phi x the sum of c over the slot's column, k_qc_mstep's chunks, its fold of the chunk's |delta|
// No float atomics; every sum one thread's in index order or one workgroup's strided partial sums folded by q_block_sum; no sum spans two
// cells.  Lanes of k_qcm_seg and k_qcm_row have uneven segment and row lengths, as k_qm_seg's and k_qm_row's do (DESIGN.md section 7).
// What follows a kernel's `done` test is quant_model.inc's body of the same name (qm_gh_sum .. qm_coefs; a stored zero's QC_NONE is tested here).
namespace {
constexpr u64 QCM_X_BYTES = 64;      // device bytes the models add per expanded non-zero: ten 4-byte tables and the segments' two 8-byte ones, besides ...
constexpr u64 QCM_COEF_BYTES = 8;    // ... a coefficient per set bit (at most H to a non-zero) and, a batch having no more slots than non-zeros, ...
constexpr u64 QCM_SLOT_BYTES = 40;   // ... the group tables per slot (slot_group, gptr, gmem, group_cell, long_groups; Phi_g, Phi_t) and ...
constexpr u64 QCM_SLOT_TABLES = 1;   // ... this many slots x H x 8-byte tables (Phi_gh)
u64 qcm_x_bytes(u32 n_haps) { return QCM_X_BYTES + QCM_SLOT_BYTES + (QCM_COEF_BYTES + QCM_SLOT_TABLES * 8) * n_haps; }

__global__ __launch_bounds__(TPB) void k_qcm_popc(const u32* x_mask, u32 n_x, u32* bits) {
    const u64 x = blockIdx.x * (u64)TPB + threadIdx.x;
    if (x < n_x) bits[x] = (u32)__popc(x_mask[x]);
}
// element i of the column view is expanded non-zero vals[i]: where its coefficients start
__global__ __launch_bounds__(TPB) void k_qcm_colb0(const u32* vals, const u32* x_b0, u32 n_x, u32* col_b0) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n_x) col_b0[i] = x_b0[vals[i]];
}
__global__ __launch_bounds__(TPB) void k_qcm_skeys(const u32* slot_cell, const u32* slot_locus, const int* gene, u32 n_slots, u64* keys, u32* vals) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s >= n_slots) return;
    keys[s] = ((u64)slot_cell[s] << 32) | (u32)gene[slot_locus[s]];
    vals[s] = (u32)s;
}
// position p of the slots sorted on (cell, gene): the member there; a group's cell at its head (gid = the exclusive scan of the heads)
__global__ __launch_bounds__(TPB) void k_qcm_groups(const u64* keys, const u32* vals, const u32* flag, const u32* gid, u32 n_slots, u32* gmem, u32* group_cell) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x;
    if (p >= n_slots) return;
    gmem[p] = vals[p];
    if (flag[p]) group_cell[gid[p]] = (u32)(keys[p] >> 32);
}
__global__ __launch_bounds__(TPB) void k_qcm_glist(const u32* gptr, u32 n_groups, u32* n_long, u32* long_groups) {
    const u64 g = blockIdx.x * (u64)TPB + threadIdx.x;
    if (g < n_groups && gptr[g + 1] - gptr[g] > Q_LONG_GENE) long_groups[atomicAdd(n_long, 1u)] = (u32)g;
}
// expanded non-zero x: key = (entry, the group of its slot), behind every group when it has no slot; value = x
__global__ __launch_bounds__(TPB) void k_qcm_rkeys(const u32* x_ent, const u32* row_slot, const u32* slot_group, u32 n_x, u32 n_groups, u64* keys, u32* vals) {
    const u64 x = blockIdx.x * (u64)TPB + threadIdx.x;
    if (x >= n_x) return;
    const u32 s = row_slot[x];
    keys[x] = ((u64)x_ent[x] << 32) | (s == QC_NONE ? n_groups : slot_group[s]);
    vals[x] = (u32)x;
}
// position p of the gene-ordered view: the expanded non-zero there; a segment's group (QC_NONE: the one of the stored zeros) and cell at its head
__global__ __launch_bounds__(TPB) void k_qcm_seginfo(const u64* keys, const u32* vals, const u32* flag, const u32* segid, const u32* ent_cell, u32 n_x,
                                                     u32 n_groups, u32* gx, u32* seg_group, u32* seg_cell) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x;
    if (p >= n_x) return;
    gx[p] = vals[p];
    if (!flag[p]) return;
    const u32 s = segid[p], g = (u32)keys[p];
    seg_group[s] = g == n_groups ? QC_NONE : g;
    seg_cell[s] = ent_cell[(u32)(keys[p] >> 32)];
}
// thread i = g H + h: Phi_gh over the members of group g in index order (loci ascending); phi is slots x H
__global__ __launch_bounds__(TPB) void k_qcm_gh(const u32* done, const u32* group_cell, const u32* gptr, const u32* gmem, const double* phi, u32 n_groups,
                                                u32 n_haps, double* phi_gh) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= (u64)n_groups * n_haps) return;
    const u32 g = (u32)(i / n_haps), h = (u32)(i - (u64)g * n_haps);
    if (done[group_cell[g]]) return;
    qm_gh_sum(gptr, gmem, phi, g, h, n_haps, phi_gh + i);
}
// workgroup b: long group long_groups[b], k_qm_ghlong's scheme
__global__ __launch_bounds__(TPB) void k_qcm_ghlong(const u32* done, const u32* group_cell, const u32* long_groups, const u32* gptr, const u32* gmem,
                                                    const double* phi, u32 n_haps, u32 hp, double* phi_gh) {
    __shared__ double s[TPB];
    const u32 g = long_groups[blockIdx.x];
    if (done[group_cell[g]]) return;
    qm_ghlong_sum(s, gptr, gmem, phi, g, n_haps, hp, phi_gh);
}
// thread i < n_groups: Phi_g = Phi_gh added over h in order; thread n_groups + s, when phi_t is asked for (model 2): Phi_t of slot s likewise
__global__ __launch_bounds__(TPB) void k_qcm_g(const u32* done, const u32* group_cell, const u32* slot_cell, const double* phi_gh, const double* phi,
                                               u32 n_groups, u32 n_slots, u32 n_haps, double* phi_g, double* phi_t) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const bool is_group = i < n_groups;
    if (!is_group && (!phi_t || i - n_groups >= n_slots)) return;
    if (done[is_group ? group_cell[i] : slot_cell[i - n_groups]]) return;
    (is_group ? phi_g[i] : phi_t[i - n_groups]) = qm_hap_sum(is_group ? phi_gh + i * n_haps : phi + (i - n_groups) * n_haps, n_haps);
}
// thread s: segment s = the positions [seg_start[s], seg_start[s + 1]) of the gene-ordered view, all of one entry and one group (models 2
// and 3; k_qm_seg's definitions, a slot for a target)
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qcm_seg(const u32* done, const u32* seg_cell, const u32* seg_group, const u32* seg_start, u32 n_segs, const u32* gx,
                                                 const u32* row_slot, const u32* x_mask, const double* phi, const double* phi_g, const double* phi_t,
                                                 u32 n_haps, double* seg_c, double* seg_x) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s >= n_segs || done[seg_cell[s]]) return;
    const u32 g = seg_group[s];
    double d = 0.0, x = 0.0;
    if (g != QC_NONE) qm_seg_sums<MODEL>(seg_start[s], seg_start[s + 1], gx, row_slot, x_mask, phi, phi_t, n_haps, d, x);
    seg_c[s] = d > 0.0 ? phi_g[g] : 0.0;
    seg_x[s] = MODEL == 2 ? x : d;
}
// model 1, thread s hp + h: k_qm_seg1's scheme.  No lane leaves before the shuffle; a workgroup none of whose segments is running leaves whole
__global__ __launch_bounds__(TPB) void k_qcm_seg1(const u32* done, const u32* seg_cell, const u32* seg_group, const u32* seg_start, u32 n_segs, const u32* gx,
                                                  const u32* row_slot, const u32* x_mask, const u32* x_b0, const double* phi, const double* phi_gh,
                                                  const double* phi_g, u32 n_haps, u32 hp, double* seg_c, double* seg_x, double* coef) {
    const u64 s = (blockIdx.x * (u64)TPB + threadIdx.x) / hp;
    const u32 h = threadIdx.x & (hp - 1u);
    const bool run = s < n_segs && !done[seg_cell[s]];
    if (!__syncthreads_or(run)) return;
    const bool on = run && h < n_haps;
    u32 a = 0, b = 0, g = QC_NONE;
    if (on) {
        g = seg_group[s];
        if (g != QC_NONE) { a = seg_start[s]; b = seg_start[s + 1]; }
    }
    qm_seg1_lanes(on, s, a, b, g, h, gx, row_slot, x_mask, x_b0, phi, phi_gh, phi_g, n_haps, hp, seg_c, seg_x, coef);
}
// thread k: entry k when it is a short row of a running cell; expl[k] = 1 when its reads were explained
__global__ __launch_bounds__(TPB) void k_qcm_row(const u32* done, const u32* ent_cell, const u32* off, u32 n_ent, const u32* segid, const double* seg_x,
                                                 const int* data_n, u32 j0, double* seg_c, uint8_t* expl) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k >= n_ent) return;
    const u32 a = off[k], b = off[k + 1];
    if (b == a || !(b - a <= QC_LONG_ROW) || done[ent_cell[k]]) return;
    expl[k] = qm_row_short((u64)data_n[j0 + k], segid[a], segid[b], seg_x, seg_c) != 0;
}
// workgroup b: long entry long_rows[b], k_qm_rowlong's scheme
__global__ __launch_bounds__(TPB) void k_qcm_rowlong(const u32* done, const u32* ent_cell, const u32* long_rows, const u32* off, const u32* segid,
                                                     const double* seg_x, const int* data_n, u32 j0, double* seg_c, uint8_t* expl) {
    __shared__ double s[TPB];
    const u32 k = long_rows[blockIdx.x];
    if (done[ent_cell[k]]) return;
    const u64 got = qm_row_long(s, (u64)data_n[j0 + k], segid[off[k]], segid[off[k + 1]], seg_x, seg_c);
    if (threadIdx.x == 0) expl[k] = got != 0;
}
// thread x: expanded non-zero x -- the coefficients of its set bits from its segment's c (k_qm_coef's definitions)
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qcm_coef(const u32* done, const u32* seg_cell, u32 n_x, const u32* x_seg, const u32* row_slot, const u32* x_mask,
                                                  const u32* x_b0, const double* phi, const double* phi_t, const double* seg_c, u32 n_haps, double* coef) {
    const u64 x = blockIdx.x * (u64)TPB + threadIdx.x;
    if (x >= n_x) return;
    const u32 sg = x_seg[x];
    if (done[seg_cell[sg]]) return;
    qm_coefs<MODEL>(seg_c, sg, row_slot, x, x_mask[x], x_b0[x], phi, phi_t, n_haps, coef);
}
// M-step, workgroup b: long column long_cols[b] (a slot), k_qm_mlong's scheme
__global__ __launch_bounds__(TPB) void k_qcm_mlong(const u32* done, const u32* slot_cell, const u32* long_cols, const u32* slot_ptr, const u32* col_b0,
                                                   const u32* col_mask, const double* coef, u32 n_haps, u32 hp, double* acc_long) {
    __shared__ double s[TPB];
    __shared__ u32 msk[TPB], b0[TPB];
    const u32 t = long_cols[blockIdx.x];
    if (done[slot_cell[t]]) return;
    const double acc = q_col_fold(s, b0, msk, col_mask, slot_ptr[t], slot_ptr[t + 1], hp, [&](u32 k) { return col_b0[k]; },
                                  [&](u32 x, u32 m, u32 h) { return qm_coef_at(coef, x, m, h); });
    if (threadIdx.x < n_haps) acc_long[(u64)t * n_haps + threadIdx.x] = acc;
}
// M-step, workgroup q: chunk q of one cell, k_qc_mstep's items: lane i one (slot, h) -- the coefficients of the slot's column entries with
// bit h, in index order (entry order); theta', the next phi, and the chunk's part of the cell's delta
__global__ __launch_bounds__(TPB) void k_qcm_mstep(const u32* done, const u32* chunk_cell, const u32* chunk_ptr, const u32* cell_slot0, const u32* slot_ptr,
                                                   const u32* col_b0, const u32* col_mask, const double* coef, const double* acc_long, const double* scale,
                                                   u32 n_haps, double* theta, double* phi, double* partial) {
    __shared__ double s[TPB];
    const u32 c = chunk_cell[blockIdx.x];
    if (done[c]) return;
    const u64 item = (u64)(blockIdx.x - chunk_ptr[c]) * TPB + threadIdx.x;
    const u64 i = (u64)cell_slot0[c] * n_haps + item;
    double diff = 0.0;
    if (item < (u64)(cell_slot0[c + 1] - cell_slot0[c]) * n_haps) {
        const u32 t = (u32)(i / n_haps), h = (u32)(i - (u64)t * n_haps);
        const u32 a = slot_ptr[t], b = slot_ptr[t + 1];
        double acc = 0.0;
        if (b - a > QC_LONG_COL) acc = acc_long[i];
        else
            for (u32 k = a; k < b; ++k) {
                const u32 m = col_mask[k];
                if ((m >> h) & 1u) acc += qm_coef_at(coef, col_b0[k], m, h);
            }
        diff = q_theta_next<false>(acc, i, scale, theta, phi);
    }
    diff = q_block_sum(diff, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = diff;
}

// The models' part of a batch's set-up.  s still holds the sort that made the slots: its values are the column view's expanded non-zeros.
int qcm_setup(Call& c, QcBufs& q, const QcView& v, const QModel& mdl, SortBufs& s, const SortScratch& ss, u32* sums, QcmTabs& t) {
    hipStream_t st = v.st;
    const u32 n_x = v.n_x, n_slots = v.n_slots;
    u64* tot = q.get<u64>(4);                                          // [0] groups, [1] segments, [2] set bits, [3] the long groups' counter
    t.x_b0 = q.get<u32>((u64)n_x + 1); t.col_b0 = q.get<u32>(n_x);
    t.slot_group = q.get<u32>(n_slots); t.gptr = q.get<u32>((u64)n_slots + 1); t.gmem = q.get<u32>(n_slots); t.group_cell = q.get<u32>(n_slots);
    t.long_groups = q.get<u32>(n_slots / Q_LONG_GENE + 1);
    u32* gid = q.get<u32>((u64)n_slots + 1);
    t.segid = q.get<u32>((u64)n_x + 1); t.seg_start = q.get<u32>((u64)n_x + 1); t.seg_group = q.get<u32>(n_x); t.seg_cell = q.get<u32>(n_x);
    t.gx = q.get<u32>(n_x); t.x_seg = q.get<u32>(n_x);
    t.seg_c = q.get<double>(n_x); t.seg_x = q.get<double>(n_x);
    if (q.short_of) return fail(nullptr, ECB_ERR_HIP, "%sout of device memory", c.prefix);
    CALLCHK(c, hipMemsetAsync(tot, 0, 32, st));
    // where the coefficients of every expanded non-zero start, in both views
    k_qcm_popc<<<nblk(n_x, TPB), TPB, 0, st>>>(v.x_mask, n_x, v.flag);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, v.flag, n_x, t.x_b0, sums, tot + 2, 1, t.x_b0 + n_x));
    k_qcm_colb0<<<nblk(n_x, TPB), TPB, 0, st>>>(s.vals(), t.x_b0, n_x, t.col_b0);
    CALLCHK(c, hipGetLastError());
    // the groups: the slots sorted on (cell, gene)
    k_qcm_skeys<<<nblk(n_slots, TPB), TPB, 0, st>>>(v.slot_cell, v.slot_locus, mdl.gene, n_slots, s.k[0], s.v[0]);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, radix_sort_pairs64(st, s, n_slots, ss, msb_mask(v.nc - 1) << 32 | msb_mask(mdl.n_genes - 1)));
    k_run_heads<<<nblk(n_slots, TPB), TPB, 0, st>>>(s.keys(), n_slots, v.flag);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, v.flag, n_slots, gid, sums, tot, 1, gid + n_slots));
    k_qm_segs<<<nblk((u64)n_slots + 1, TPB), TPB, 0, st>>>(v.flag, gid, s.vals(), n_slots, t.gptr, t.slot_group);
    k_qcm_groups<<<nblk(n_slots, TPB), TPB, 0, st>>>(s.keys(), s.vals(), v.flag, gid, n_slots, t.gmem, t.group_cell);
    CALLCHK(c, hipGetLastError());
    u64 back[4];
    if (const int rc = c.read_back(back, tot, 4)) return rc;
    t.n_groups = (u32)back[0];
    if (back[2] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant-cells: one cell alone holds 2^32 set haplotype bits or more");
    k_qcm_glist<<<nblk(t.n_groups, TPB), TPB, 0, st>>>(t.gptr, t.n_groups, reinterpret_cast<u32*>(tot + 3), t.long_groups);
    // the segments: the expanded non-zeros sorted on (entry, group)
    k_qcm_rkeys<<<nblk(n_x, TPB), TPB, 0, st>>>(v.x_ent, v.row_slot, t.slot_group, n_x, t.n_groups, s.k[0], s.v[0]);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, radix_sort_pairs64(st, s, n_x, ss, msb_mask(v.n_ent - 1) << 32 | msb_mask(t.n_groups)));
    k_run_heads<<<nblk(n_x, TPB), TPB, 0, st>>>(s.keys(), n_x, v.flag);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, v.flag, n_x, t.segid, sums, tot + 1, 1, t.segid + n_x));
    k_qm_segs<<<nblk((u64)n_x + 1, TPB), TPB, 0, st>>>(v.flag, t.segid, s.vals(), n_x, t.seg_start, t.x_seg);
    k_qcm_seginfo<<<nblk(n_x, TPB), TPB, 0, st>>>(s.keys(), s.vals(), v.flag, t.segid, v.ent_cell, n_x, t.n_groups, t.gx, t.seg_group, t.seg_cell);
    CALLCHK(c, hipGetLastError());
    if (const int rc = c.read_back(back, tot, 4)) return rc;
    t.n_segs = (u32)back[1];
    t.n_long_groups = (u32)back[3];
    t.phi_gh = q.get<double>((u64)t.n_groups * v.n_haps); t.phi_g = q.get<double>(t.n_groups);
    t.phi_t = mdl.model == 2u ? q.get<double>(n_slots) : nullptr;
    t.coef = q.get<double>(back[2]);
    if (q.short_of) return fail(nullptr, ECB_ERR_HIP, "%sout of device memory", c.prefix);
    return ECB_OK;
}

void qcm_step(const QcView& v, const QcmTabs& t, u32 model) {
    hipStream_t st = v.st;
    const u32 H = v.n_haps;
    k_qcm_gh<<<nblk((u64)t.n_groups * H, TPB), TPB, 0, st>>>(v.done, t.group_cell, t.gptr, t.gmem, v.phi, t.n_groups, H, t.phi_gh);
    if (t.n_long_groups) k_qcm_ghlong<<<t.n_long_groups, TPB, 0, st>>>(v.done, t.group_cell, t.long_groups, t.gptr, t.gmem, v.phi, H, v.hp, t.phi_gh);
    k_qcm_g<<<nblk((u64)t.n_groups + (t.phi_t ? v.n_slots : 0u), TPB), TPB, 0, st>>>(v.done, t.group_cell, v.slot_cell, t.phi_gh, v.phi, t.n_groups, v.n_slots, H,
                                                                                      t.phi_g, t.phi_t);
    if (model == 1u)
        k_qcm_seg1<<<nblk((u64)t.n_segs * v.hp, TPB), TPB, 0, st>>>(v.done, t.seg_cell, t.seg_group, t.seg_start, t.n_segs, t.gx, v.row_slot, v.x_mask, t.x_b0,
                                                                    v.phi, t.phi_gh, t.phi_g, H, v.hp, t.seg_c, t.seg_x, t.coef);
    else if (model == 2u)
        k_qcm_seg<2><<<nblk(t.n_segs, TPB), TPB, 0, st>>>(v.done, t.seg_cell, t.seg_group, t.seg_start, t.n_segs, t.gx, v.row_slot, v.x_mask, v.phi, t.phi_g,
                                                          t.phi_t, H, t.seg_c, t.seg_x);
    else
        k_qcm_seg<3><<<nblk(t.n_segs, TPB), TPB, 0, st>>>(v.done, t.seg_cell, t.seg_group, t.seg_start, t.n_segs, t.gx, v.row_slot, v.x_mask, v.phi, t.phi_g,
                                                          t.phi_t, H, t.seg_c, t.seg_x);
    if (v.nlr) k_qcm_rowlong<<<v.nlr, TPB, 0, st>>>(v.done, v.ent_cell, v.long_rows, v.off, t.segid, t.seg_x, v.data_n, v.j0, t.seg_c, v.expl);
    k_qcm_row<<<nblk(v.n_ent, TPB), TPB, 0, st>>>(v.done, v.ent_cell, v.off, v.n_ent, t.segid, t.seg_x, v.data_n, v.j0, t.seg_c, v.expl);
    if (model == 1u)
        k_qcm_coef<1><<<nblk(v.n_x, TPB), TPB, 0, st>>>(v.done, t.seg_cell, v.n_x, t.x_seg, v.row_slot, v.x_mask, t.x_b0, v.phi, t.phi_t, t.seg_c, H, t.coef);
    else if (model == 2u)
        k_qcm_coef<2><<<nblk(v.n_x, TPB), TPB, 0, st>>>(v.done, t.seg_cell, v.n_x, t.x_seg, v.row_slot, v.x_mask, t.x_b0, v.phi, t.phi_t, t.seg_c, H, t.coef);
    else
        k_qcm_coef<3><<<nblk(v.n_x, TPB), TPB, 0, st>>>(v.done, t.seg_cell, v.n_x, t.x_seg, v.row_slot, v.x_mask, t.x_b0, v.phi, t.phi_t, t.seg_c, H, t.coef);
    if (v.nlc) k_qcm_mlong<<<v.nlc, TPB, 0, st>>>(v.done, v.slot_cell, v.long_cols, v.slot_ptr, t.col_b0, v.col_mask, t.coef, H, v.hp, v.acc_long);
    k_qcm_mstep<<<v.nq, TPB, 0, st>>>(v.done, v.chunk_cell, v.chunk_ptr, v.cell_slot0, v.slot_ptr, t.col_b0, v.col_mask, t.coef, v.acc_long, v.scale, H,
                                      v.theta, v.phi, v.partial);
}

// what both entry points refuse before anything else (then ecb_quantify_cells's own checks)
int qcm_check_args(uint32_t n_loci, uint32_t n_genes, const void* gene, uint32_t model) {
    if (model < 1u || model > 4u) return fail(nullptr, ECB_ERR_ARG, "ecquant-cells: no such model (%u: 1, 2, 3 or 4)", model);
    if (!gene || (n_loci && !n_genes)) return fail(nullptr, ECB_ERR_ARG, "ecquant-cells: bad argument (no gene array, or targets and no gene)");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_quantify_cells_model_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                               const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                               const void* d_indices_n, const void* d_data_n, const void* d_cell_keep, const void* d_scale,
                                               const void* d_theta_in, uint32_t max_iters, double tol, uint64_t budget_bytes, uint32_t n_genes,
                                               const void* d_gene, uint32_t model, uint64_t n_slots, void* d_cell_ptr, void* d_slot_locus, void* d_theta,
                                               void* d_n_iter, void* d_delta, void* d_explained, void* d_converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(qcm_check_args(n_loci, n_genes, d_gene, model));
    RCCHK(qc_check_quant(m, d_cell_ptr, d_slot_locus, d_theta, n_slots, tol));
    const QModel mdl{model, n_genes, (const int*)d_gene};
    return qc_run(true, device, m, d_cell_keep, d_scale, d_theta_in, max_iters, tol, budget_bytes, n_slots,
                  QcOut{d_cell_ptr, d_slot_locus, d_theta, d_n_iter, d_delta, d_explained, d_converged}, nullptr, &mdl);
}

extern "C" int ecb_quantify_cells_model(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                                        const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                        const int32_t* indices_n, const int32_t* data_n, const uint8_t* cell_keep, const double* scale,
                                        const double* theta_in, uint32_t max_iters, double tol, uint64_t budget_bytes, uint32_t n_genes, const int32_t* gene,
                                        uint32_t model, uint64_t n_slots, int64_t* cell_ptr, int32_t* slot_locus, double* theta, uint32_t* n_iter,
                                        double* delta, int64_t* explained, uint8_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(qcm_check_args(n_loci, n_genes, gene, model));
    RCCHK(qc_check_quant(m, cell_ptr, slot_locus, theta, n_slots, tol));
    const QModel mdl{model, n_genes, gene};
    return qc_host(device, m, cell_keep, scale, theta_in, max_iters, tol, budget_bytes, &mdl, n_slots, cell_ptr, slot_locus, theta, n_iter, delta, explained,
                   converged);
}

