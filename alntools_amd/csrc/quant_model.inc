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
namespace {
constexpr u32 Q_LONG_GENE = 32;      // a gene with more members than this has its Phi_gh summed by a workgroup, not by a lane per haplotype
enum : u32 { Q_ERR_GENE = 4u };
const ErrBit QM_ERRS[] = {
    {Q_ERR_SCALE, ECB_ERR_CONTRACT, "ecquant: an entry of scale is NaN, infinite or negative"},
    {Q_ERR_THETA, ECB_ERR_CONTRACT, "ecquant: an entry of theta_in is NaN, infinite or negative"},
    {Q_ERR_GENE, ECB_ERR_CONTRACT, "ecquant: a gene id outside [0, n_genes)"},
};
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
// thread i = g H + h: Phi_gh over the members of g in index order (loci ascending)
__global__ __launch_bounds__(TPB) void k_qm_gh(const QState* st, const int* gptr, const int* gmem, const double* phi, u32 n_genes, u32 n_haps,
                                               double* phi_gh) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= (u64)n_genes * n_haps) return;
    const u32 g = (u32)(i / n_haps), h = (u32)(i - (u64)g * n_haps);
    const u32 a = (u32)gptr[g], b = (u32)gptr[g + 1];
    if (b - a > Q_LONG_GENE) return;
    double s = 0.0;
    for (u32 k = a; k < b; ++k) s += phi[(u64)gmem[k] * n_haps + h];
    phi_gh[i] = s;
}
// workgroup b: long gene long_genes[b] -- thread k, haplotype k % hp (hp: the power of two at or above H), adds members k / hp, k / hp +
// TPB / hp, ...; the tree folds the TPB / hp sums of a haplotype
__global__ __launch_bounds__(TPB) void k_qm_ghlong(const QState* st, const u32* long_genes, const int* gptr, const int* gmem, const double* phi,
                                                   u32 n_haps, u32 hp, double* phi_gh) {
    __shared__ double s[TPB];
    if (st->done) return;
    const u32 g = long_genes[blockIdx.x], h = threadIdx.x & (hp - 1u), slot = threadIdx.x / hp, stride = TPB / hp;
    const u32 a = (u32)gptr[g], b = (u32)gptr[g + 1];
    double acc = 0.0;
    if (h < n_haps)
        for (u32 k = a + slot; k < b; k += stride) acc += phi[(u64)gmem[k] * n_haps + h];
    acc = q_block_sum(acc, s, hp);
    if (threadIdx.x < n_haps) phi_gh[(u64)g * n_haps + threadIdx.x] = acc;
}
// thread i < G: Phi_g = Phi_gh added over h in order; thread G + t, when phi_t is asked for (model 2): Phi_t = phi[., t] likewise
__global__ __launch_bounds__(TPB) void k_qm_g(const QState* st, const double* phi_gh, const double* phi, u32 n_genes, u32 n_loci, u32 n_haps,
                                              double* phi_g, double* phi_t) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    const bool is_gene = i < n_genes;
    if (!is_gene && (!phi_t || i - n_genes >= n_loci)) return;
    const double* p = is_gene ? phi_gh + i * n_haps : phi + (i - n_genes) * n_haps;
    double s = 0.0;
    for (u32 h = 0; h < n_haps; ++h) s += p[h];
    (is_gene ? phi_g[i] : phi_t[i - n_genes]) = s;
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
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p], t = (u32)indices[i], m = (u32)data[i];
        if (MODEL == 2) {
            const double dt = q_bits_sum(phi, n_haps, t, m, 0.0);
            d += dt;
            if (dt > 0.0) x += phi_t[t];
        } else d = q_bits_sum(phi, n_haps, t, m, d);
    }
    seg_c[s] = d > 0.0 ? phi_g[(u32)rkeys[a]] : 0.0;
    seg_x[s] = MODEL == 2 ? x : d;
}
// model 1, thread s hp + h (hp: the power of two at or above H, so a wave holds whole segments): D_h of segment s over its non-zeros with
// bit h, in index order; Phi_gh / D_h left at the place of each such bit's coefficient; the allele denominator = the Phi_gh of the lanes
// with D_h > 0 added in h order (every lane of the segment adds the same values in the same order)
__global__ __launch_bounds__(TPB) void k_qm_seg1(const QState* st, const u32* seg_start, u32 n_segs, const u64* rkeys, const u32* gnz, const int* indices,
                                                 const int* data, const u32* bits_excl, const double* phi, const double* phi_gh, const double* phi_g,
                                                 u32 n_haps, u32 hp, double* seg_c, double* seg_x, double* coef) {
    if (st->done) return;
    const u64 s = (blockIdx.x * (u64)TPB + threadIdx.x) / hp;
    const u32 h = threadIdx.x & (hp - 1u), bit = 1u << h;
    const bool on = s < n_segs && h < n_haps;
    u32 a = 0, b = 0, g = 0;
    if (on) { a = seg_start[s]; b = seg_start[s + 1]; g = (u32)rkeys[a]; }
    double dh = 0.0;
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p];
        if ((u32)data[i] & bit) dh += phi[(u64)indices[i] * n_haps + h];
    }
    const double pg = dh > 0.0 ? phi_gh[(u64)g * n_haps + h] : 0.0, f = dh > 0.0 ? pg / dh : 0.0;
    double x = 0.0;
    for (u32 k = 0; k < n_haps; ++k) x += __shfl(pg, (int)k, (int)hp);
    for (u32 p = a; p < b; ++p) {
        const u32 i = gnz[p], m = (u32)data[i];
        if (m & bit) coef[bits_excl[i] + __popc(m & (bit - 1u))] = f;
    }
    if (on && h == 0u) { seg_c[s] = x > 0.0 ? phi_g[g] : 0.0; seg_x[s] = x; }
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
// thread e: the short rows; parts[b] = the weights workgroup b explained
__global__ __launch_bounds__(TPB) void k_qm_row(const QState* st, const int* indptr, u32 n_ecs, const u32* segid, const double* seg_x, const u64* ww,
                                                double* seg_c, u64* parts) {
    __shared__ u64 s[TPB];
    if (st->done) return;
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    u64 got = 0;
    if (e < n_ecs) {
        const u32 a = (u32)indptr[e], b = (u32)indptr[e + 1];
        if (b - a <= Q_LONG_ROW) {
            const u32 s0 = segid[a], s1 = segid[b];
            double r;
            q_row_done(ww[e], qm_gene_sum(seg_c, s0, s1, 0, 1), &r, got);
            qm_seg_coefs(seg_c, seg_x, r, s0, s1, 0, 1);
        }
    }
    got = q_block_sum(got, s);
    if (threadIdx.x == 0) parts[blockIdx.x] = got;
}
// workgroup b: long row long_rows[b] -- thread k adds segments k, k + TPB, ... in that order, the tree folds the TPB sums; then thread k
// gives the same segments their coefficients
__global__ __launch_bounds__(TPB) void k_qm_rowlong(const QState* st, const u32* long_rows, const int* indptr, const u32* segid, const double* seg_x,
                                                    const u64* ww, double* seg_c, u64* parts) {
    __shared__ double s[TPB];
    if (st->done) return;
    const u32 e = long_rows[blockIdx.x];
    const u32 s0 = segid[indptr[e]], s1 = segid[indptr[e + 1]];
    const double gd = q_block_sum(qm_gene_sum(seg_c, s0, s1, threadIdx.x, TPB), s);
    double r;
    u64 got;
    q_row_done(ww[e], gd, &r, got);
    qm_seg_coefs(seg_c, seg_x, r, s0, s1, threadIdx.x, TPB);
    if (threadIdx.x == 0) parts[blockIdx.x] = got;
}
// thread i: non-zero i, in storage order -- the coefficients of its set bits from its segment's c
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qm_coef(const QState* st, u64 nnz, const u32* nz_seg, const int* indices, const int* data, const u32* bits_excl,
                                                 const double* phi, const double* phi_t, const double* seg_c, u32 n_haps, double* coef) {
    if (st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= nnz) return;
    const u32 m = (u32)data[i], b0 = bits_excl[i], n = (u32)__popc(m);
    const double c = seg_c[nz_seg[i]];
    if (MODEL == 1) {
        for (u32 j = 0; j < n; ++j) coef[b0 + j] = c * coef[b0 + j];
    } else {
        double cv = c;
        if (MODEL == 2) {
            const u32 t = (u32)indices[i];
            const double dt = q_bits_sum(phi, n_haps, t, m, 0.0);
            cv = dt > 0.0 ? c * phi_t[t] / dt : 0.0;
        }
        for (u32 j = 0; j < n; ++j) coef[b0 + j] = cv;
    }
}
// the coefficient of bit h of a column entry with mask m whose coefficients start at b0
__device__ __forceinline__ double qm_coef_at(const double* coef, u32 b0, u32 m, u32 h) { return coef[b0 + __popc(m & ((1u << h) - 1u))]; }
// M-step, workgroup b: long column long_cols[b], as k_q_mlong: thread k stages entry k's mask and base, then with haplotype k % hp adds of
// the entries k / hp, k / hp + TPB / hp, ... the coefficients of those with its bit
__global__ __launch_bounds__(TPB) void k_qm_mlong(const QState* st, const u32* long_cols, const int* colptr, const u32* col_b0, const int* col_mask,
                                                  const double* coef, u32 n_haps, u32 hp, double* acc_long) {
    __shared__ double s[TPB];
    __shared__ u32 msk[TPB], b0[TPB];
    if (st->done) return;
    const u32 t = long_cols[blockIdx.x], h = threadIdx.x & (hp - 1u), slot = threadIdx.x / hp, stride = TPB / hp;
    const u32 a = (u32)colptr[t], b = (u32)colptr[t + 1];
    double acc = 0.0;
    for (u32 base = a; base < b; base += TPB) {
        const u32 n = std::min<u32>(TPB, b - base);
        if (threadIdx.x < n) { msk[threadIdx.x] = (u32)col_mask[base + threadIdx.x]; b0[threadIdx.x] = col_b0[base + threadIdx.x]; }
        __syncthreads();
        for (u32 j = slot; j < n; j += stride)
            if ((msk[j] >> h) & 1u) acc += qm_coef_at(coef, b0[j], msk[j], h);
        __syncthreads();
    }
    acc = q_block_sum(acc, s, hp);
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
        const double was = theta[i], now = phi[i] * acc;
        theta[i] = now;
        phi[i] = scale ? now * scale[i] : now;
        diff = fabs(now - was);
    }
    diff = q_block_sum(diff, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = diff;
}
// what both entry points refuse before anything else (then q_check_args)
int qm_check_args(uint32_t n_loci, uint32_t n_haps, uint32_t n_genes, const void* gene, uint32_t model) {
    if (model < 1u || model > 4u) return fail(nullptr, ECB_ERR_ARG, "ecquant: no such model (%u: 1, 2, 3 or 4)", model);
    if (!gene || (n_loci && !n_genes)) return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no gene array, or targets and no gene)");
    if ((u64)n_genes * n_haps >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x genes does not fit 31 bits");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_quantify_model_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                         const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                         const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                                         uint32_t max_iters, double tol, uint32_t n_genes, const void* d_gene, uint32_t model, void* d_theta,
                                         uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    RCCHK(qm_check_args(n_loci, n_haps, n_genes, d_gene, model));
    RCCHK(q_check_args(n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, sample, tol,
                       d_theta));
    const int* gene = (const int*)d_gene;
    if (model == 4u) {
        // the flat step is ecb_quantify's own: the genes are checked, then it runs as it always has
        {
            Call c(device, "ecquant: "); if (c.rc) return c.rc;
            u64* word = c.get<u64>(1);
            if (const int rc = c.missing()) return rc;
            CALLCHK(c, hipMemsetAsync(word, 0, 8, c.st));
            if (n_loci) k_qm_gkeys<<<nblk(n_loci, TPB), TPB, 0, c.st>>>(gene, n_loci, n_genes, nullptr, nullptr, reinterpret_cast<u32*>(word));
            CALLCHK(c, hipGetLastError());
            u64 back = 0;
            if (const int rc = c.read_back(&back, word, 1, QM_ERRS)) return rc;
        }
        return ecb_quantify_device(device, n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, n_samples, nnz_n, d_indptr_n, d_indices_n,
                                   d_data_n, sample, d_scale, d_theta_in, max_iters, tol, d_theta, n_iter, delta, explained, converged);
    }
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);          // as ecb_quantify_device: [5] gains the error bit of gene
    const u64 n_tab = (u64)n_haps * n_loci, n_gtab = (u64)n_haps * n_genes;
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *bits = c.get<u32>(CV_X0, nnz), *bits_excl = c.get<u32>(CV_X1, nnz + 1), *sums = c.get<u32>(CV_SUMS2, scan_words(nnz + 1));
    u64* ww = c.get<u64>(CV_X2, n_ecs);
    double *theta = c.get<double>(n_tab), *phi = c.get<double>(n_tab), *scale = d_scale ? c.get<double>(n_tab) : nullptr;
    u64 *gk0 = c.get<u64>(n_loci), *gk1 = c.get<u64>(n_loci);
    u32 *gv0 = c.get<u32>(n_loci), *gv1 = c.get<u32>(n_loci);
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
    if (d_scale) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_scale, n_loci, n_haps, scale, Q_ERR_SCALE, reinterpret_cast<u32*>(words + 5));
    if (d_theta_in) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_theta_in, n_loci, n_haps, theta, Q_ERR_THETA, reinterpret_cast<u32*>(words + 5));
    if (n_loci) k_qm_gkeys<<<nblk(n_loci, TPB), TPB, 0, st>>>(gene, n_loci, n_genes, gk0, gv0, reinterpret_cast<u32*>(words + 5));
    CALLCHK(c, hipGetLastError());
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    if (back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    RCCHK(refuse_bits(nullptr, QM_ERRS, (u32)back[5]));
    // the input is well formed: from here on the outputs are written
    const u64 n_bits = back[3];
    QState fin{};
    fin.converged = 1u;
    if (!n_ecs || !nnz) CALLCHK(c, hipMemsetAsync(d_theta, 0, n_tab * 8, st));
    else {
        u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
        u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
        SortScratch ss{c.get<u32>(CV_HIST, rs_words(std::max<u64>(nnz, n_loci))), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 4};
        int *colptr = c.get<int>((u64)n_loci + 1), *col_ec = c.get<int>(nnz), *col_mask = c.get<int>(nnz);
        u32* col_b0 = c.get<u32>(nnz);
        u32 *long_rows = c.get<u32>(nnz / Q_LONG_ROW + 1), *long_cols = c.get<u32>(nnz / Q_LONG_COL + 1);
        u32* long_genes = c.get<u32>(n_loci / Q_LONG_GENE + 1);
        int *gptr = c.get<int>((u64)n_genes + 1), *gmem = c.get<int>(n_loci);
        u32 *flag = c.get<u32>(nnz), *segid = c.get<u32>(nnz + 1), *seg_start = c.get<u32>(nnz + 1), *nz_seg = c.get<u32>(nnz);
        const u32 n_parts = nblk(n_tab, TPB);
        const u32 n_eblk = nblk(n_ecs, TPB);
        double *acc_long = c.get<double>(n_tab), *partial = c.get<double>(n_parts);
        double *phi_gh = c.get<double>(n_gtab), *phi_g = c.get<double>(n_genes), *phi_t = model == 2u ? c.get<double>(n_loci) : nullptr;
        double *seg_c = c.get<double>(nnz), *seg_x = c.get<double>(nnz), *coef = c.get<double>(n_bits);
        u64* expl_parts = c.get<u64>((u64)n_eblk + nnz / Q_LONG_ROW + 1);          // the short rows' workgroups, then the long rows'
        QState* qs = c.get<QState>(1);
        u64* n_segs_d = c.get<u64>(1);
        u32* n_long_genes_d = c.get<u32>(1);
        if (const int rc = c.missing()) return rc;
        CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QState), st));
        CALLCHK(c, hipMemsetAsync(n_long_genes_d, 0, 4, st));
        // the members of each gene: the targets sorted by gene, stable, so loci ascend within one
        SortBufs sg{{gk0, gk1}, {gv0, gv1}};
        CALLCHK(c, radix_sort_pairs64(st, sg, n_loci, ss, msb_mask(n_genes - 1) << 32));
        k_split_out<<<nblk(n_loci, TPB), TPB, 0, st>>>(sg.keys(), sg.vals(), n_loci, gmem, gmem);                  // (index and value are both the target)
        k_row_ptr<<<nblk((u64)n_genes + 1, TPB), TPB, 0, st>>>(sg.keys(), n_loci, n_genes, gptr);
        k_qm_glist<<<nblk(n_genes, TPB), TPB, 0, st>>>(gptr, n_genes, n_long_genes_d, long_genes);
        // the column view, as ecb_quantify_device builds it, and where each entry's coefficients start
        k_cv_keys<<<nblk(n_ecs, TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, n_loci, n_haps, k0, v0, reinterpret_cast<u32*>(words + 6));
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_loci - 1) << 32));
        k_split_out<<<nblk(nnz, TPB), TPB, 0, st>>>(s.keys(), s.vals(), nnz, col_ec, col_mask);
        k_row_ptr<<<nblk((u64)n_loci + 1, TPB), TPB, 0, st>>>(s.keys(), nnz, n_loci, colptr);
        k_qm_colbase<<<nblk(nnz, TPB), TPB, 0, st>>>(s.keys(), nnz, ip, ix, bits_excl, col_b0);
        // the gene-ordered view of the rows, its segments (the sorted keys stay: row and gene of every position)
        k_qm_rkeys<<<nblk(n_ecs, TPB), TPB, 0, st>>>(ip, n_ecs, ix, gene, k0, v0);
        CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_ecs - 1) << 32 | msb_mask(n_genes - 1)));
        const u64* rkeys = s.keys(); const u32* gnz = s.vals();
        k_run_heads<<<nblk(nnz, TPB), TPB, 0, st>>>(rkeys, nnz, flag);
        CALLCHK(c, scan_launch(st, flag, nnz, segid, sums, n_segs_d, 1, segid + nnz));
        k_qm_segs<<<nblk(nnz + 1, TPB), TPB, 0, st>>>(flag, segid, gnz, nnz, seg_start, nz_seg);
        k_q_rows<<<n_eblk, TPB, 0, st>>>(ip, n_ecs, bits_excl, ww, qs, long_rows, expl_parts);
        k_q_w<<<1, TPB, 0, st>>>(qs, expl_parts, n_eblk);
        k_q_cols<<<nblk(n_loci, TPB), TPB, 0, st>>>(colptr, n_loci, qs, long_cols);
        CALLCHK(c, hipGetLastError());
        QState q0;
        u64 n_segs64 = 0;
        u32 nlg = 0;
        CALLCHK(c, hipMemcpyAsync(&q0, qs, sizeof(QState), hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipMemcpyAsync(&n_segs64, n_segs_d, 8, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipMemcpyAsync(&nlg, n_long_genes_d, 4, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
        const u32 nlr = q0.n_long_rows, nlc = q0.n_long_cols, n_segs = (u32)n_segs64;
        u32 hp = 1;
        while (hp < n_haps) hp <<= 1;
        k_q_arm<<<1, 1, 0, st>>>(qs, max_iters, tol * (double)q0.W);
        if (d_theta_in) k_q_phi<<<nblk(n_tab, TPB), TPB, 0, st>>>(theta, scale, n_tab, phi);
        else {
            if (nlc) k_q_mlong<true><<<nlc, TPB, 0, st>>>(qs, long_cols, colptr, col_ec, col_mask, nullptr, ww, n_haps, hp, acc_long);
            k_q_mstep<true><<<n_parts, TPB, 0, st>>>(qs, colptr, col_ec, col_mask, nullptr, ww, acc_long, scale, n_loci, n_haps, theta, phi, partial);
        }
        CALLCHK(c, hipGetLastError());
        fin = QState{};
        fin.done = max_iters == 0u;
        for (u32 queued = 0; !fin.done;) {
            for (u32 k = 0; k < Q_BATCH && queued < max_iters; ++k, ++queued) {
                k_qm_gh<<<nblk(n_gtab, TPB), TPB, 0, st>>>(qs, gptr, gmem, phi, n_genes, n_haps, phi_gh);
                if (nlg) k_qm_ghlong<<<nlg, TPB, 0, st>>>(qs, long_genes, gptr, gmem, phi, n_haps, hp, phi_gh);
                k_qm_g<<<nblk((u64)n_genes + (phi_t ? n_loci : 0u), TPB), TPB, 0, st>>>(qs, phi_gh, phi, n_genes, n_loci, n_haps, phi_g, phi_t);
                if (model == 1u)
                    k_qm_seg1<<<nblk((u64)n_segs * hp, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, bits_excl, phi, phi_gh, phi_g, n_haps, hp,
                                                                          seg_c, seg_x, coef);
                else if (model == 2u)
                    k_qm_seg<2><<<nblk(n_segs, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, phi, phi_g, phi_t, n_haps, seg_c, seg_x);
                else k_qm_seg<3><<<nblk(n_segs, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, phi, phi_g, phi_t, n_haps, seg_c, seg_x);
                if (nlr) k_qm_rowlong<<<nlr, TPB, 0, st>>>(qs, long_rows, ip, segid, seg_x, ww, seg_c, expl_parts + n_eblk);
                k_qm_row<<<n_eblk, TPB, 0, st>>>(qs, ip, n_ecs, segid, seg_x, ww, seg_c, expl_parts);
                if (model == 1u) k_qm_coef<1><<<nblk(nnz, TPB), TPB, 0, st>>>(qs, nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, coef);
                else if (model == 2u) k_qm_coef<2><<<nblk(nnz, TPB), TPB, 0, st>>>(qs, nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, coef);
                else k_qm_coef<3><<<nblk(nnz, TPB), TPB, 0, st>>>(qs, nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, coef);
                if (nlc) k_qm_mlong<<<nlc, TPB, 0, st>>>(qs, long_cols, colptr, col_b0, col_mask, coef, n_haps, hp, acc_long);
                k_qm_mstep<<<n_parts, TPB, 0, st>>>(qs, colptr, col_b0, col_mask, coef, acc_long, scale, n_loci, n_haps, theta, phi, partial);
                k_q_conv<<<1, TPB, 0, st>>>(qs, partial, n_parts, expl_parts, n_eblk + nlr);
            }
            CALLCHK(c, hipGetLastError());
            CALLCHK(c, hipMemcpyAsync(&fin, qs, sizeof(QState), hipMemcpyDeviceToHost, st));
            CALLCHK(c, hipStreamSynchronize(st));
        }
        k_q_out<<<nblk(n_tab, TPB), TPB, 0, st>>>(theta, n_loci, n_haps, (double*)d_theta);
        CALLCHK(c, hipGetLastError());
    }
    CALLCHK(c, hipStreamSynchronize(st));
    if (n_iter) *n_iter = fin.n_iter;
    if (delta) *delta = fin.delta;
    if (explained) *explained = (int64_t)fin.explained;
    if (converged) *converged = fin.converged;
    return ECB_OK;
}

extern "C" int ecb_quantify_model(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                                  const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                  const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                                  uint32_t max_iters, double tol, uint32_t n_genes, const int32_t* gene, uint32_t model, double* theta,
                                  uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    RCCHK(qm_check_args(n_loci, n_haps, n_genes, gene, model));
    RCCHK(q_check_args(n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n, sample, tol, theta));
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    const u64 plane = (u64)n_haps * n_loci * 8;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, sc, ti, gn, out;
    std::vector<StageIn> in = {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz * 4}, {&daa, data_a, nnz * 4},
                               {&ipn, indptr_n, ((u64)n_samples + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4},
                               {&gn, gene, (u64)n_loci * 4}, {&out, nullptr, plane}};
    if (scale) in.push_back({&sc, scale, plane});
    if (theta_in) in.push_back({&ti, theta_in, plane});
    int rc = stage_in(c, in);
    uint32_t it = 0, conv = 0; double dl = 0.0; int64_t ex = 0;
    if (rc == ECB_OK) rc = ecb_quantify_model_device(device, n_ecs, n_loci, n_haps, nnz, ipa.p, ixa.p, daa.p, n_samples, nnz_n, ipn.p, ixn.p, dan.p,
                                                     sample, sc.p, ti.p, max_iters, tol, n_genes, gn.p, model, out.p, &it, &dl, &ex, &conv);
    RCCHK(rc);
    RCCHK(stage_out(c, {{theta, &out, plane}}));
    if (n_iter) *n_iter = it;
    if (delta) *delta = dl;
    if (explained) *explained = ex;
    if (converged) *converged = conv;
    return ECB_OK;
}
