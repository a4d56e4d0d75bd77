// ---- ecquant's hierarchical models over a gene grouping (ecb_quantify_model / ecb_quantify_model_device; included by ecb.hip after quant.inc)
// (AlignmentPropertyMatrix.normalize_reads(axis=LOCUS | GROUP | HAPLOGROUP, grouping_mat=...) and bundle(reset=True),
//  AlignmentPropertyMatrix.py:219-275 and 340-384, composed as EMASE composes them: model 1 gene -> allele -> isoform, model 2 gene ->
//  isoform -> allele, model 3 gene -> isoform x allele; model 4, the flat step, is ecb_quantify itself.)
// A row's posterior at (t, h) is a product of factors whose sums run over subsets of the row's set bits: the bits of one gene (a SEGMENT of
// the row), of one gene and haplotype, of one non-zero.  Once per call the non-zeros are put into (row, gene, locus) order by the library's
// stable radix sort -- they come in (row, locus) order, so the sort on (row, gene[t]) leaves the genes of a row as contiguous segments with
// loci ascending inside them; the value is the non-zero's index -- and the segment starts are marked and scanned.  The members of each gene
// are a CSR built by the same sort (loci ascending).  The column view of ecquant gains, per entry, where its non-zero's coefficients start.
// One step, every sum by one thread in index order or by one workgroup with q_block_sum's fixed tree, no float atomics, no scatter of sums:
//   k_qm_gh [k_qm_ghlong]   Phi_gh = the sum of phi[h, t] over the members of g (a gene with more than Q_LONG_GENE members: a workgroup)
//   k_qm_g                  Phi_g = the sum of Phi_gh over h; model 2: Phi_t = the sum of phi[h, t] over h
//   k_qm_seg / k_qm_seg1    per segment: whether it is alive (D > 0: then Phi_g is its term of the row's gene denominator) and what its
//                           coefficient is divided by -- model 3: D = the sum of phi over its set bits; model 2: the isoform denominator
//                           (the sum of Phi_t over its non-zeros with D_t > 0); model 1, hp lanes to a segment, one per haplotype: D_h, the
//                           allele denominator (the sum of Phi_gh over the h with D_h > 0), and Phi_gh / D_h left at each bit's place
//   [k_qm_rowlong] k_qm_row per row: the gene denominator (the sum of Phi_g over its live segments), w over it, the explained weight; each of
//                           its segments gets c = w x Phi_g / the gene denominator / the segment's divisor
//   k_qm_coef               per non-zero, in storage order: one coefficient per set bit, w x (the factors) / phi[h, t], at bits_excl[nz] + the
//                           set bits below h -- model 3: c; model 2: c x Phi_t / D_t; model 1: c x what k_qm_seg1 left there
//   [k_qm_mlong] k_qm_mstep theta'[h, t] = phi[h, t] x the sum of c over the column's entries with bit h, in column order; delta's parts
//   k_q_conv                unchanged
// A member whose own D is 0 is left out of every denominator (DESIGN.md section 7: where the reference keeps it, mass is lost).
// The kernels' bodies after their early-exit test (qm_gh_sum, qm_ghlong_sum, qm_hap_sum, qm_seg_sums, qm_seg1_lanes, qm_row_short, qm_row_long,
// qm_coefs; the M-step's are quant.inc's q_col_fold and q_theta_next) are shared with the per-cell copies of quant_cells_model.inc.  Host side:
// qm_gene_view (the members' CSR, the long genes, the gene-ordered view and its segments), qm_setup and qm_step are what quant.inc's q_run
// plugs in for a model, and what ecb_posterior_device (quant_post.inc) runs once; qm_check_genes is model 4's check of the gene ids alone.
namespace {
constexpr u32 Q_LONG_GENE = 32;      // a gene with more members than this has its Phi_gh summed by a workgroup, not by a lane per haplotype
// target t: its gene checked; key = gene << 32 | t for the members' CSR
__global__ __launch_bounds__(TPB) void k_qm_gkeys(const int* gene, u32 n_loci, u32 n_genes, u64* keys, u32* vals, u32* err) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t >= n_loci) return;
    u32 g = (u32)gene[t];
    if (g >= n_genes) { atomicOr(err, Q_ERR_GENE); g = 0; }
    if (keys) { keys[t] = ((u64)g << 32) | (u32)t; vals[t] = (u32)t; }
}
// one thread per row: key = row << 32 | the gene of the non-zero's target, value = the non-zero's index
__global__ __launch_bounds__(TPB) void k_qm_rkeys(const int* indptr, u32 n_ecs, const int* indices, const int* gene, u64* keys, u32* vals) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e >= n_ecs) return;
    for (u32 i = (u32)indptr[e], b = (u32)indptr[e + 1]; i < b; ++i) {
        keys[i] = (e << 32) | (u32)gene[indices[i]];
        vals[i] = i;
    }
}
// segid = the exclusive scan of the segment heads (nnz + 1 values): segment s starts at the head p with segid[p] = s, the last one ends at
// nnz; nz_seg = the segment of every non-zero (gnz: the non-zero at position p of the gene-ordered view)
__global__ __launch_bounds__(TPB) void k_qm_segs(const u32* flag, const u32* segid, const u32* gnz, u64 nnz, u32* seg_start, u32* nz_seg) {
    const u64 p = blockIdx.x * (u64)TPB + threadIdx.x;
    if (p < nnz) {
        if (flag[p]) seg_start[segid[p]] = (u32)p;
        nz_seg[gnz[p]] = segid[p + 1] - 1u;
    } else if (p == nnz) seg_start[segid[nnz]] = (u32)nnz;
}
// column entry k = (locus << 32 | row) of the column view: col_b0[k] = bits_excl of its non-zero (found in its row by bisection)
__global__ __launch_bounds__(TPB) void k_qm_colbase(const u64* ckeys, u64 nnz, const int* indptr, const int* indices, const u32* bits_excl, u32* col_b0) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k >= nnz) return;
    const u32 e = (u32)ckeys[k];
    const int t = (int)(ckeys[k] >> 32);
    u32 lo = (u32)indptr[e], hi = (u32)indptr[e + 1];
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (indices[m] < t) lo = m + 1; else hi = m; }
    col_b0[k] = bits_excl[lo];
}
__global__ __launch_bounds__(TPB) void k_qm_glist(const int* gptr, u32 n_genes, u32* n_long, u32* long_genes) {
    const u64 g = blockIdx.x * (u64)TPB + threadIdx.x;
    if (g < n_genes && (u32)(gptr[g + 1] - gptr[g]) > Q_LONG_GENE) long_genes[atomicAdd(n_long, 1u)] = (u32)g;
}
// The gene sums (k_qm_gh, k_qm_ghlong, k_qm_g and their k_qcm_* twins, where a gene is a (cell, gene) group and a target a slot).
// Phi_gh of (g, h) over the members of g in index order (loci ascending), unless g is long
template <class P> __device__ __forceinline__ void qm_gh_sum(const P* gptr, const P* gmem, const double* phi, u32 g, u32 h, u32 n_haps, double* out) {
    const u32 a = (u32)gptr[g], b = (u32)gptr[g + 1];
    if (b - a > Q_LONG_GENE) return;
    double s = 0.0;
    for (u32 k = a; k < b; ++k) s += phi[(u64)gmem[k] * n_haps + h];
    *out = s;
}
// a workgroup, long gene g: thread k, haplotype k % hp (hp: the power of two at or above H), adds members k / hp, k / hp + TPB / hp, ...; the
// tree folds the TPB / hp sums of a haplotype
template <class P>
__device__ __forceinline__ void qm_ghlong_sum(double* s, const P* gptr, const P* gmem, const double* phi, u32 g, u32 n_haps, u32 hp, double* phi_gh) {
    const u32 h = threadIdx.x & (hp - 1u), slot = threadIdx.x / hp, stride = TPB / hp;
    const u32 a = (u32)gptr[g], b = (u32)gptr[g + 1];
    double acc = 0.0;
    if (h < n_haps)
        for (u32 k = a + slot; k < b; k += stride) acc += phi[(u64)gmem[k] * n_haps + h];
    acc = q_block_sum(acc, s, hp);
    if (threadIdx.x < n_haps) phi_gh[(u64)g * n_haps + threadIdx.x] = acc;
}
// the H values at p added in h order
__device__ __forceinline__ double qm_hap_sum(const double* p, u32 n_haps) {
    double s = 0.0;
    for (u32 h = 0; h < n_haps; ++h) s += p[h];
    return s;
}
// thread i = g H + h: Phi_gh over the members of g
__global__ __launch_bounds__(TPB) void k_qm_gh(const QState* st, const int* gptr, const int* gmem, const double* phi, u32 n_genes, u32 n_haps,
                                               double* phi_gh) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= (u64)n_genes * n_haps) return;
    const u32 g = (u32)(i / n_haps), h = (u32)(i - (u64)g * n_haps);
    qm_gh_sum(gptr, gmem, phi, g, h, n_haps, phi_gh + i);
}
// workgroup b: long gene long_genes[b]
__global__ __launch_bounds__(TPB) void k_qm_ghlong(const QState* st, const u32* long_genes, const int* gptr, const int* gmem, const double* phi,
                                                   u32 n_haps, u32 hp, double* phi_gh) {
    __shared__ double s[TPB];
    if (st->done) return;
    qm_ghlong_sum(s, gptr, gmem, phi, long_genes[blockIdx.x], n_haps, hp, phi_gh);
}
// thread i < G: Phi_g = Phi_gh added over h in order; thread G + t, when phi_t is asked for (model 2): Phi_t = phi[., t] likewise
__global__ __launch_bounds__(TPB) void k_qm_g(const QState* st, const double* phi_gh, const double* phi, u32 n_genes, u32 n_loci, u32 n_haps,
                                              double* phi_g, double* phi_t) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const bool is_gene = i < n_genes;
    if (!is_gene && (!phi_t || i - n_genes >= n_loci)) return;
    (is_gene ? phi_g[i] : phi_t[i - n_genes]) = qm_hap_sum(is_gene ? phi_gh + i * n_haps : phi + (i - n_genes) * n_haps, n_haps);
}
// The sums of one segment, the positions [a, b) of the gene-ordered view (gnz: the non-zero there; it gathers at where[i] with mask[i]), for
// models 2 and 3 (k_qm_seg, k_qcm_seg): d = the phi of its set bits -- model 2: non-zero by non-zero, and x = the Phi_t of those with D_t > 0
template <u32 MODEL, class I>
__device__ __forceinline__ void qm_seg_sums(u32 a, u32 b, const u32* gnz, const I* where, const I* mask, const double* phi, const double* phi_t,
                                            u32 n_haps, double& d, double& x) {
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p], t = (u32)where[i], m = (u32)mask[i];
        if (MODEL == 2) {
            const double dt = q_bits_sum(phi, n_haps, t, m, 0.0);
            d += dt;
            if (dt > 0.0) x += phi_t[t];
        } else d = q_bits_sum(phi, n_haps, t, m, d);
    }
}
// Model 1's segment, hp lanes to it (k_qm_seg1, k_qcm_seg1; every lane of the wave calls this, `on` or not: a = b for one that is not): lane
// h's D_h over the segment's non-zeros with bit h, in index order; Phi_gh / D_h left at the place of each such bit's coefficient (b0[i] + the
// set bits below h); the allele denominator = the Phi_gh of the lanes with D_h > 0 added in h order (every lane of the segment adds the same
// values in the same order); lane 0 writes the segment's term and divisor
template <class I>
__device__ __forceinline__ void qm_seg1_lanes(bool on, u64 s, u32 a, u32 b, u32 g, u32 h, const u32* gnz, const I* where, const I* mask, const u32* b0,
                                              const double* phi, const double* phi_gh, const double* phi_g, u32 n_haps, u32 hp, double* seg_c,
                                              double* seg_x, double* coef) {
    const u32 bit = 1u << h;
    double dh = 0.0;
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p];
        if ((u32)mask[i] & bit) dh += phi[(u64)where[i] * n_haps + h];
    }
    const double pg = dh > 0.0 ? phi_gh[(u64)g * n_haps + h] : 0.0, f = dh > 0.0 ? pg / dh : 0.0;
    double x = 0.0;
    for (u32 k = 0; k < n_haps; ++k) x += __shfl(pg, (int)k, (int)hp);
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p], m = (u32)mask[i];
        if (m & bit) coef[b0[i] + __popc(m & (bit - 1u))] = f;
    }
    if (on && h == 0u) { seg_c[s] = x > 0.0 ? phi_g[g] : 0.0; seg_x[s] = x; }
}
// thread s: segment s = the positions [seg_start[s], seg_start[s + 1]) of the gene-ordered view, all of one row and one gene (models 2 and 3).
// seg_c = Phi_g when the segment is alive, else 0: its term of the row's gene denominator; seg_x = what its coefficient is divided by
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qm_seg(const QState* st, const u32* seg_start, u32 n_segs, const u64* rkeys, const u32* gnz, const int* indices,
                                                const int* data, const double* phi, const double* phi_g, const double* phi_t, u32 n_haps,
                                                double* seg_c, double* seg_x) {
    if (st->done) return;
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s >= n_segs) return;
    const u32 a = seg_start[s], b = seg_start[s + 1];
    double d = 0.0, x = 0.0;
    qm_seg_sums<MODEL>(a, b, gnz, indices, data, phi, phi_t, n_haps, d, x);
    seg_c[s] = d > 0.0 ? phi_g[(u32)rkeys[a]] : 0.0;
    seg_x[s] = MODEL == 2 ? x : d;
}
// model 1, thread s hp + h (hp: the power of two at or above H, so a wave holds whole segments): qm_seg1_lanes
__global__ __launch_bounds__(TPB) void k_qm_seg1(const QState* st, const u32* seg_start, u32 n_segs, const u64* rkeys, const u32* gnz, const int* indices,
                                                 const int* data, const u32* bits_excl, const double* phi, const double* phi_gh, const double* phi_g,
                                                 u32 n_haps, u32 hp, double* seg_c, double* seg_x, double* coef) {
    if (st->done) return;
    const u64 s = (blockIdx.x * (u64)TPB + threadIdx.x) / hp;
    const u32 h = threadIdx.x & (hp - 1u);
    const bool on = s < n_segs && h < n_haps;
    u32 a = 0, b = 0, g = 0;
    if (on) { a = seg_start[s]; b = seg_start[s + 1]; g = (u32)rkeys[a]; }
    qm_seg1_lanes(on, s, a, b, g, h, gnz, indices, data, bits_excl, phi, phi_gh, phi_g, n_haps, hp, seg_c, seg_x, coef);
}
// the segments [s0, s1) of a row, every `step`-th from s0 + first: their terms of the gene denominator added up ...
__device__ __forceinline__ double qm_gene_sum(const double* seg_c, u32 s0, u32 s1, u32 first, u32 step) {
    double gd = 0.0;
    for (u32 s = s0 + first; s < s1; s += step) gd += seg_c[s];
    return gd;
}
// ... and, with r = w over that sum, each live segment's c = r x Phi_g / its divisor in place of its term
__device__ __forceinline__ void qm_seg_coefs(double* seg_c, const double* seg_x, double r, u32 s0, u32 s1, u32 first, u32 step) {
    for (u32 s = s0 + first; s < s1; s += step) {
        const double pg = seg_c[s];
        seg_c[s] = pg > 0.0 ? r * pg / seg_x[s] : 0.0;
    }
}
// A short row's segments [s0, s1), by its lane (k_qm_row, k_qcm_row): the gene denominator, r = w over it, the segments' coefficients;
// the weight explained comes back
__device__ __forceinline__ u64 qm_row_short(u64 w, u32 s0, u32 s1, const double* seg_x, double* seg_c) {
    double r;
    u64 got;
    q_row_done(w, qm_gene_sum(seg_c, s0, s1, 0, 1), &r, got);
    qm_seg_coefs(seg_c, seg_x, r, s0, s1, 0, 1);
    return got;
}
// A long row's, by its workgroup (k_qm_rowlong, k_qcm_rowlong): thread k adds segments k, k + TPB, ... in that order, the tree folds the TPB
// sums; then thread k gives the same segments their coefficients (every thread of the workgroup calls this; thread 0's return counts)
__device__ __forceinline__ u64 qm_row_long(double* s, u64 w, u32 s0, u32 s1, const double* seg_x, double* seg_c) {
    const double gd = q_block_sum(qm_gene_sum(seg_c, s0, s1, threadIdx.x, TPB), s);
    double r;
    u64 got;
    q_row_done(w, gd, &r, got);
    qm_seg_coefs(seg_c, seg_x, r, s0, s1, threadIdx.x, TPB);
    return got;
}
// thread e: the short rows; parts[b] = the weights workgroup b explained
__global__ __launch_bounds__(TPB) void k_qm_row(const QState* st, const int* indptr, u32 n_ecs, const u32* segid, const double* seg_x, const u64* ww,
                                                double* seg_c, u64* parts) {
    __shared__ u64 s[TPB];
    if (st->done) return;
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    u64 got = 0;
    if (e < n_ecs) {
        const u32 a = (u32)indptr[e], b = (u32)indptr[e + 1];
        if (b - a <= Q_LONG_ROW) got = qm_row_short(ww[e], segid[a], segid[b], seg_x, seg_c);
    }
    got = q_block_sum(got, s);
    if (threadIdx.x == 0) parts[blockIdx.x] = got;
}
// workgroup b: long row long_rows[b]
__global__ __launch_bounds__(TPB) void k_qm_rowlong(const QState* st, const u32* long_rows, const int* indptr, const u32* segid, const double* seg_x,
                                                    const u64* ww, double* seg_c, u64* parts) {
    __shared__ double s[TPB];
    if (st->done) return;
    const u32 e = long_rows[blockIdx.x];
    const u64 got = qm_row_long(s, ww[e], segid[indptr[e]], segid[indptr[e + 1]], seg_x, seg_c);
    if (threadIdx.x == 0) parts[blockIdx.x] = got;
}
// The coefficients of non-zero i (gathering at where[i], its mask m, its coefficients from b0 on) from the c of its segment sg (k_qm_coef,
// k_qcm_coef): model 3: c; model 2: c x Phi_t / D_t; model 1: c x what the segment kernel left there.  (A stored mask of 0 has no coefficient,
// and in the cells nowhere to gather.)
template <u32 MODEL, class I>
__device__ __forceinline__ void qm_coefs(const double* seg_c, u32 sg, const I* where, u64 i, u32 m, u32 b0, const double* phi, const double* phi_t,
                                         u32 n_haps, double* coef) {
    const u32 n = (u32)__popc(m);
    const double c = seg_c[sg];
    if (MODEL == 1) {
        for (u32 j = 0; j < n; ++j) coef[b0 + j] = c * coef[b0 + j];
    } else {
        double cv = c;
        if (MODEL == 2 && m) {
            const u32 t = (u32)where[i];
            const double dt = q_bits_sum(phi, n_haps, t, m, 0.0);
            cv = dt > 0.0 ? c * phi_t[t] / dt : 0.0;
        }
        for (u32 j = 0; j < n; ++j) coef[b0 + j] = cv;
    }
}
// thread i: non-zero i, in storage order -- the coefficients of its set bits from its segment's c
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qm_coef(const QState* st, u64 nnz, const u32* nz_seg, const int* indices, const int* data, const u32* bits_excl,
                                                 const double* phi, const double* phi_t, const double* seg_c, u32 n_haps, double* coef) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= nnz) return;
    qm_coefs<MODEL>(seg_c, nz_seg[i], indices, i, (u32)data[i], bits_excl[i], phi, phi_t, n_haps, coef);
}
// the coefficient of bit h of a column entry with mask m whose coefficients start at b0
__device__ __forceinline__ double qm_coef_at(const double* coef, u32 b0, u32 m, u32 h) { return coef[b0 + __popc(m & ((1u << h) - 1u))]; }
// M-step, workgroup b: long column long_cols[b], as k_q_mlong: q_col_fold over where its entries' coefficients start
__global__ __launch_bounds__(TPB) void k_qm_mlong(const QState* st, const u32* long_cols, const int* colptr, const u32* col_b0, const int* col_mask,
                                                  const double* coef, u32 n_haps, u32 hp, double* acc_long) {
    __shared__ double s[TPB];
    __shared__ u32 msk[TPB], b0[TPB];
    if (st->done) return;
    const u32 t = long_cols[blockIdx.x];
    const double acc = q_col_fold(s, b0, msk, col_mask, (u32)colptr[t], (u32)colptr[t + 1], hp, [&](u32 k) { return col_b0[k]; },
                                  [&](u32 x, u32 m, u32 h) { return qm_coef_at(coef, x, m, h); });
    if (threadIdx.x < n_haps) acc_long[(u64)t * n_haps + threadIdx.x] = acc;
}
// M-step, thread i = t H + h: the coefficients of column t's entries with bit h, in index order (ascending EC); theta', the next phi, and
// the workgroup's part of delta
__global__ __launch_bounds__(TPB) void k_qm_mstep(const QState* st, const int* colptr, const u32* col_b0, const int* col_mask, const double* coef,
                                                  const double* acc_long, const double* scale, u32 n_loci, u32 n_haps, double* theta, double* phi,
                                                  double* partial) {
    __shared__ double s[TPB];
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    double diff = 0.0;
    if (i < (u64)n_loci * n_haps) {
        const u32 t = (u32)(i / n_haps), h = (u32)(i - (u64)t * n_haps);
        const u32 a = (u32)colptr[t], b = (u32)colptr[t + 1];
        double acc = 0.0;
        if (b - a > Q_LONG_COL) acc = acc_long[i];
        else
            for (u32 k = a; k < b; ++k) {
                const u32 m = (u32)col_mask[k];
                if ((m >> h) & 1u) acc += qm_coef_at(coef, col_b0[k], m, h);
            }
        diff = q_theta_next<false>(acc, i, scale, theta, phi);
    }
    diff = q_block_sum(diff, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = diff;
}
// what the model and the posterior entry points refuse before anything else (then q_check_args)
int qm_check_args(uint32_t n_loci, uint32_t n_haps, uint32_t n_genes, const void* gene, uint32_t model) {
    if (model < 1u || model > 4u) return fail(nullptr, ECB_ERR_ARG, "ecquant: no such model (%u: 1, 2, 3 or 4)", model);
    if (!gene || (n_loci && !n_genes)) return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no gene array, or targets and no gene)");
    if ((u64)n_genes * n_haps >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x genes does not fit 31 bits");
    return ECB_OK;
}
// model 4 is the flat step, but its gene ids are refused like the others': checked in a call of their own, before the flat run starts
int qm_check_genes(int device, const char* prefix, const int* gene, u32 n_loci, u32 n_genes) {
    Call c(device, prefix); if (c.rc) return c.rc;
    u64* word = c.get<u64>(1);
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemsetAsync(word, 0, 8, c.st));
    if (n_loci) k_qm_gkeys<<<nblk(n_loci, TPB), TPB, 0, c.st>>>(gene, n_loci, n_genes, nullptr, nullptr, reinterpret_cast<u32*>(word));
    CALLCHK(c, hipGetLastError());
    u64 back = 0;
    return c.read_back(&back, word, 1, Q_ERRS);
}
// The gene view.  The members of each gene: the targets sorted by gene (the front's keys), stable, so loci ascend within one; the genes
// above Q_LONG_GENE listed.  The gene-ordered view of the rows: the non-zeros sorted on (row, gene), stable -- it stays in srt's buffers
// (row and gene of every position, the non-zero there) --, its run heads scanned = the segments.  Enqueued only: the two counts stay on
// the device for the caller to read
int qm_gene_view(Call& c, const QMat& m, const QFront& f, const int* gene, u32 n_genes, QSort& srt, QGenes& g) {
    hipStream_t st = c.st;
    const u64 nnz = m.nnz;
    const u32 n_loci = m.n_loci;
    g = QGenes{};
    g.n_genes = n_genes;
    g.gptr = c.get<int>((u64)n_genes + 1); g.gmem = c.get<int>(n_loci); g.long_genes = c.get<u32>(n_loci / Q_LONG_GENE + 1);
    u32* flag = c.get<u32>(nnz);
    g.segid = c.get<u32>(nnz + 1); g.seg_start = c.get<u32>(nnz + 1); g.nz_seg = c.get<u32>(nnz);
    g.cnt = c.get<u64>(2);
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemsetAsync(g.cnt + 1, 0, 8, st));
    SortBufs sg{{f.gk[0], f.gk[1]}, {f.gv[0], f.gv[1]}};
    CALLCHK(c, radix_sort_pairs64(st, sg, n_loci, srt.ss, msb_mask(n_genes - 1) << 32));
    k_split_out<<<nblk(n_loci, TPB), TPB, 0, st>>>(sg.keys(), sg.vals(), n_loci, g.gmem, g.gmem);                  // (index and value are both the target)
    k_row_ptr<<<nblk((u64)n_genes + 1, TPB), TPB, 0, st>>>(sg.keys(), n_loci, n_genes, g.gptr);
    k_qm_glist<<<nblk(n_genes, TPB), TPB, 0, st>>>(g.gptr, n_genes, reinterpret_cast<u32*>(g.cnt + 1), g.long_genes);
    k_qm_rkeys<<<nblk(m.n_ecs, TPB), TPB, 0, st>>>(m.ip, m.n_ecs, m.ix, gene, srt.s.k[0], srt.s.v[0]);
    CALLCHK(c, radix_sort_pairs64(st, srt.s, nnz, srt.ss, msb_mask(m.n_ecs - 1) << 32 | msb_mask(n_genes - 1)));
    g.rkeys = srt.s.keys(); g.gnz = srt.s.vals();
    k_run_heads<<<nblk(nnz, TPB), TPB, 0, st>>>(g.rkeys, nnz, flag);
    CALLCHK(c, scan_launch(st, flag, nnz, g.segid, f.sums, g.cnt, 1, g.segid + nnz));
    k_qm_segs<<<nblk(nnz + 1, TPB), TPB, 0, st>>>(flag, g.segid, g.gnz, nnz, g.seg_start, g.nz_seg);
    CALLCHK(c, hipGetLastError());
    return ECB_OK;
}
// the chain's tables (coef: where the coefficients go; null: a buffer of the call's)
int qm_tables(Call& c, const QMat& m, const QFront& f, const QModel& mdl, double* coef, QmTabs& t) {
    t.phi_gh = c.get<double>((u64)m.n_haps * mdl.n_genes); t.phi_g = c.get<double>(mdl.n_genes);
    t.phi_t = mdl.model == 2u ? c.get<double>(m.n_loci) : nullptr;
    t.seg_c = c.get<double>(m.nnz); t.seg_x = c.get<double>(m.nnz);
    t.coef = coef ? coef : c.get<double>(f.n_bits);
    return c.missing();
}
// the models' part of q_run's set-up: both
int qm_setup(Call& c, const QMat& m, const QFront& f, const QModel& mdl, QSort& srt, QmTabs& t) {
    RCCHK(qm_gene_view(c, m, f, mdl.gene, mdl.n_genes, srt, t.g));
    return qm_tables(c, m, f, mdl, nullptr, t);
}
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qp_post(u64 nnz, const u32* nz_seg, const int* indices, const int* data, const u32* bits_excl, const double* phi,
                                                 const double* phi_t, const double* seg_c, u32 n_haps, double* post);          // (quant_post.inc)
// One step of the chain, through k_qm_row; then the coefficients and the M-step -- or, post: the posterior itself in the coefficients' place
void qm_step(const QView& v, const QmTabs& t, u32 model, bool post) {
    hipStream_t st = v.st;
    const QGenes& g = t.g;
    const u32 H = v.n_haps, G = g.n_genes, n_segs = g.n_segs;
    const u64 nnz = v.nnz;
    k_qm_gh<<<nblk((u64)G * H, TPB), TPB, 0, st>>>(v.qs, g.gptr, g.gmem, v.phi, G, H, t.phi_gh);
    if (g.n_long_genes) k_qm_ghlong<<<g.n_long_genes, TPB, 0, st>>>(v.qs, g.long_genes, g.gptr, g.gmem, v.phi, H, v.hp, t.phi_gh);
    k_qm_g<<<nblk((u64)G + (t.phi_t ? v.n_loci : 0u), TPB), TPB, 0, st>>>(v.qs, t.phi_gh, v.phi, G, v.n_loci, H, t.phi_g, t.phi_t);
    if (model == 1u)
        k_qm_seg1<<<nblk((u64)n_segs * v.hp, TPB), TPB, 0, st>>>(v.qs, g.seg_start, n_segs, g.rkeys, g.gnz, v.ix, v.da, v.bits_excl, v.phi, t.phi_gh, t.phi_g, H,
                                                                 v.hp, t.seg_c, t.seg_x, t.coef);
    else if (model == 2u)
        k_qm_seg<2><<<nblk(n_segs, TPB), TPB, 0, st>>>(v.qs, g.seg_start, n_segs, g.rkeys, g.gnz, v.ix, v.da, v.phi, t.phi_g, t.phi_t, H, t.seg_c, t.seg_x);
    else k_qm_seg<3><<<nblk(n_segs, TPB), TPB, 0, st>>>(v.qs, g.seg_start, n_segs, g.rkeys, g.gnz, v.ix, v.da, v.phi, t.phi_g, t.phi_t, H, t.seg_c, t.seg_x);
    if (v.nlr) k_qm_rowlong<<<v.nlr, TPB, 0, st>>>(v.qs, v.long_rows, v.ip, g.segid, t.seg_x, v.ww, t.seg_c, v.expl_parts + v.n_eblk);
    k_qm_row<<<v.n_eblk, TPB, 0, st>>>(v.qs, v.ip, v.n_ecs, g.segid, t.seg_x, v.ww, t.seg_c, v.expl_parts);
    if (post) {
        if (model == 1u) k_qp_post<1><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
        else if (model == 2u) k_qp_post<2><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
        else k_qp_post<3><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
        return;
    }
    if (model == 1u) k_qm_coef<1><<<nblk(nnz, TPB), TPB, 0, st>>>(v.qs, nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
    else if (model == 2u) k_qm_coef<2><<<nblk(nnz, TPB), TPB, 0, st>>>(v.qs, nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
    else k_qm_coef<3><<<nblk(nnz, TPB), TPB, 0, st>>>(v.qs, nnz, g.nz_seg, v.ix, v.da, v.bits_excl, v.phi, t.phi_t, t.seg_c, H, t.coef);
    if (v.nlc) k_qm_mlong<<<v.nlc, TPB, 0, st>>>(v.qs, v.long_cols, v.cols.colptr, v.cols.col_b0, v.cols.col_mask, t.coef, H, v.hp, v.acc_long);
    k_qm_mstep<<<v.n_parts, TPB, 0, st>>>(v.qs, v.cols.colptr, v.cols.col_b0, v.cols.col_mask, t.coef, v.acc_long, v.scale, v.n_loci, H, v.theta, v.phi, v.partial);
}
}  // namespace

extern "C" int ecb_quantify_model_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                         const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                         const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                                         uint32_t max_iters, double tol, uint32_t n_genes, const void* d_gene, uint32_t model, void* d_theta,
                                         uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(qm_check_args(n_loci, n_haps, n_genes, d_gene, model));
    RCCHK(q_check_args(m, sample, tol, d_theta));
    const QModel mdl{model, n_genes, (const int*)d_gene};
    QResult res;
    RCCHK(q_run(device, m, sample, d_scale, d_theta_in, max_iters, tol, d_theta, res, &mdl));
    res.put(n_iter, delta, explained, converged);
    return ECB_OK;
}

extern "C" int ecb_quantify_model(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                                  const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                  const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                                  uint32_t max_iters, double tol, uint32_t n_genes, const int32_t* gene, uint32_t model, double* theta,
                                  uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(qm_check_args(n_loci, n_haps, n_genes, gene, model));
    RCCHK(q_check_args(m, sample, tol, theta));
    const QModel mdl{model, n_genes, gene};
    return q_host(device, m, sample, scale, theta_in, max_iters, tol, &mdl, theta, n_iter, delta, explained, converged);
}
