// ---- ecquant: EM abundance estimates of a CSR A weighted by N (ecb_quantify / ecb_quantify_device; included by ecb.hip) ------------------
// (AlignmentPropertyMatrix.multiply(axis=2) / normalize_reads(axis=READ) / sum(axis=READ), AlignmentPropertyMatrix.py:277-384, iterated.)
// One step is two gathers.  E-step: a pass over A's rows, d[e] = the sum of phi over the row's set bits, r[e] = w[e] / d[e].  M-step: a pass
// over a column-major view of A built once per call -- the non-zeros sorted by locus, stable (the conversion's k_cv_keys, the library's radix
// sort, k_split_out, k_row_ptr), so the ECs of a column ascend -- theta'[h, t] = phi[h, t] x the sum of r over the column's entries with bit
// h.  No float atomics and no scatter: every sum is taken by one thread in index order, or by one workgroup as strided partial sums folded
// by a fixed tree, so the result is a function of the inputs alone.  phi, theta and scale are kept T x H: the H values one non-zero
// gathers share a line (64 bytes at H = 8).  The gathered tables (phi: H T 8 bytes, r: E 8 bytes) are L2- or Infinity-Cache-sized.
// A row or column longer than Q_LONG_ROW / Q_LONG_COL gets a workgroup of its own (the lists are built once; their order does not matter:
// a long row's workgroup writes r[e], a long column's the sums its (h, t) threads then use in place of their own loops).  The explained
// reads and W are exact integers; they too are added without atomics (one same-address add per wave cost 0.65 ms at 3.7 M rows): a part
// per workgroup, the parts added by one workgroup.
// The stop is the device's: k_q_conv adds the workgroups' parts of delta in index order, counts the step and sets `done`; every kernel
// launched after that returns at once, so the host may enqueue Q_BATCH steps between looks and the run still ends at the exact step.
// Steps: k_ca_weights | k_gm_check<true> | k_scan_lb || read back || k_q_tab x2 | k_cv_keys, k_rs_*, k_split_out, k_row_ptr | k_q_rows,
// k_q_w, k_q_cols || read back || [theta_0 = aln: k_q_mlong<true>, k_q_mstep<true>] | per step: [k_q_elong] k_q_estep [k_q_mlong] k_q_mstep k_q_conv
// | k_q_out.
// This file also holds what the whole ecquant family shares (quant_model.inc, quant_cells.inc, quant_cells_model.inc and quant_post.inc are
// included after it).  Host side, below the kernels: q_front, the one validation front (its callers: q_run, qc_run, ecb_posterior_device);
// q_col_view, the column view; q_run, the one driver of the flat step and, with a QModel, of the models' (qm_setup / qm_step, quant_model.inc);
// q_stage / q_host / QResult, the host entry points' staging and scalars.  Device side: the bodies that kernels of several files run after their
// own indexing and early-exit test -- q_tile_pass, q_long_row_sum, q_col_fold, q_theta_next -- so that the order of every sum stands once.
namespace {
constexpr u32 Q_LONG_ROW = 256;      // a row with more non-zeros than this is summed by a workgroup, not a lane
constexpr u32 Q_LONG_COL = 32;       // a column with more entries than this likewise (its lane would wait for every entry in turn: 256 cost 0.2 ms)
constexpr u32 Q_TILE = 2048;        // k_q_estep: non-zeros of a workgroup's rows in LDS at a time
constexpr u32 Q_BATCH = 8;           // steps enqueued between two looks at the device's state
enum : u32 { Q_ERR_SCALE = 1u, Q_ERR_THETA = 2u, Q_ERR_GENE = 4u };
struct QState {
    u32 done, n_iter, converged, max_iters;
    double delta, stop;              // stop = tol x W
    u64 explained, W;                // of the last whole step; of the matrix
    u32 n_long_rows, n_long_cols;
};
const ErrBit Q_ERRS[] = {
    {Q_ERR_SCALE, ECB_ERR_CONTRACT, "ecquant: an entry of scale is NaN, infinite or negative"},
    {Q_ERR_THETA, ECB_ERR_CONTRACT, "ecquant: an entry of theta_in is NaN, infinite or negative"},
    {Q_ERR_GENE, ECB_ERR_CONTRACT, "ecquant: a gene id outside [0, n_genes)"},          // (the flat step never sets it)
};
// the workgroup's TPB values folded by a fixed tree down to `stop` sums (a power of two): thread k < stop gets back the sum of the values
// of the threads k, k + stop, k + 2 stop, ... (every thread of the workgroup calls this)
template <class V> __device__ __forceinline__ V q_block_sum(V v, V* s, u32 stop = 1) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (u32 k = TPB / 2; k >= stop; k >>= 1) {
        if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    return s[threadIdx.x < stop ? threadIdx.x : 0];
}
// in: H x T row-major as the caller holds it -> out: T x H; an entry that is NaN, infinite or negative sets `bit`
__global__ __launch_bounds__(TPB) void k_q_tab(const double* in, u32 n_loci, u32 n_haps, double* out, u32 bit, u32* err) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= (u64)n_loci * n_haps) return;
    const u32 t = (u32)(i / n_haps), h = (u32)(i - (u64)t * n_haps);
    const double v = in[(u64)h * n_loci + t];
    if (!(v >= 0.0) || v > 1.7976931348623157e308) atomicOr(err, bit);
    out[i] = v;
}
__global__ __launch_bounds__(TPB) void k_q_phi(const double* theta, const double* scale, u64 n, double* phi) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i < n) phi[i] = scale ? theta[i] * scale[i] : theta[i];
}
// row e: its weight counted into the workgroup's part of W when it holds a set bit; listed when it is long
__global__ __launch_bounds__(TPB) void k_q_rows(const int* indptr, u32 n_ecs, const u32* bits_excl, const u64* ww, QState* st, u32* long_rows,
                                                u64* parts) {
    __shared__ u64 s[TPB];
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    u64 w = 0;
    if (e < n_ecs) {
        const u32 a = (u32)indptr[e], b = (u32)indptr[e + 1];
        if (bits_excl[b] != bits_excl[a]) w = ww[e];
        if (b - a > Q_LONG_ROW) long_rows[atomicAdd(&st->n_long_rows, 1u)] = (u32)e;
    }
    w = q_block_sum(w, s);
    if (threadIdx.x == 0) parts[blockIdx.x] = w;
}
// one workgroup: the parts of an integer sum added up (thread 0 gets the sum; every thread of the workgroup calls this)
__device__ __forceinline__ u64 q_parts_sum(const u64* parts, u32 n, u64* s) {
    u64 v = 0;
    for (u32 k = threadIdx.x; k < n; k += TPB) v += parts[k];
    return q_block_sum(v, s);
}
__global__ __launch_bounds__(TPB) void k_q_w(QState* st, const u64* parts, u32 n) {
    __shared__ u64 s[TPB];
    const u64 w = q_parts_sum(parts, n, s);
    if (threadIdx.x == 0) st->W = w;
}
__global__ __launch_bounds__(TPB) void k_q_cols(const int* colptr, u32 n_loci, QState* st, u32* long_cols) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t < n_loci && (u32)(colptr[t + 1] - colptr[t]) > Q_LONG_COL) long_cols[atomicAdd(&st->n_long_cols, 1u)] = (u32)t;
}
__global__ void k_q_arm(QState* st, u32 max_iters, double stop) {
    st->max_iters = max_iters;
    st->stop = stop;
    st->done = max_iters == 0u;
}
// the phi of non-zero (t, m): its set bits, lowest first
__device__ __forceinline__ double q_bits_sum(const double* phi, u32 n_haps, u32 t, u32 m, double d) {
    const double* p = phi + (u64)t * n_haps;
    for (; m; m &= m - 1u) d += p[__ffs((int)m) - 1];
    return d;
}
__device__ __forceinline__ void q_row_done(u64 w, double d, double* r_out, u64& got) {
    *r_out = d > 0.0 ? (double)w / d : 0.0;
    got = d > 0.0 ? w : 0;
}
// The LDS tile pass of the E-step (k_q_estep, k_qc_estep, k_qp_drow).  A workgroup's TPB rows are one stretch [lo, hi) of non-zeros (where
// non-zero i gathers: where[i], its mask: mask[i]): it goes through v TILE non-zeros at a time -- thread k the phi of non-zeros k, k + TPB, ...
// of the tile (its set bits, lowest first: coalesced loads, the same work for every lane whatever the rows' lengths), then the lane whose
// row [a, b) is `mine` adds those of its row in index order.  Every thread of the workgroup calls this; a lane gets its row's sum
template <u32 TILE, class I>
__device__ __forceinline__ double q_tile_pass(double* v, const double* phi, u32 n_haps, const I* where, const I* mask, u32 lo, u32 hi, u32 a, u32 b,
                                              bool mine) {
    double d = 0.0;
    for (u32 base = lo; base < hi; base += TILE) {
        const u32 n = std::min<u32>(TILE, hi - base);
        for (u32 k = threadIdx.x; k < n; k += TPB) v[k] = q_bits_sum(phi, n_haps, (u32)where[base + k], (u32)mask[base + k], 0.0);
        __syncthreads();
        if (mine)
            for (u32 i = std::max(a, base), y = std::min(b, base + n); i < y; ++i) d += v[i - base];
        __syncthreads();
    }
    return d;
}
// The long-row sum (k_q_elong, k_qc_elong, k_qp_dlong): thread k sums non-zeros k, k + TPB, ... of [a, b) in that order, the tree folds the
// TPB sums (every thread of the workgroup calls this; thread 0 gets the sum)
template <class I>
__device__ __forceinline__ double q_long_row_sum(double* s, const double* phi, u32 n_haps, const I* where, const I* mask, u32 a, u32 b) {
    double d = 0.0;
    for (u32 i = a + threadIdx.x; i < b; i += TPB) d = q_bits_sum(phi, n_haps, (u32)where[i], (u32)mask[i], d);
    return q_block_sum(d, s);
}
// E-step, the short rows.  Workgroup b has rows [b TPB, (b + 1) TPB): q_tile_pass over their stretch of A.  parts[b] = the weights the
// workgroup explained.  The non-zeros of a long row in the stretch are staged like the others and then read by nobody (k_q_elong has
// summed them): wasted gathers, one tile per Q_TILE of them -- 94 k of config 3's 13 M non-zeros; tiles that lie inside a long row are not
// skipped.
__global__ __launch_bounds__(TPB) void k_q_estep(const QState* st, const int* indptr, u32 n_ecs, const int* indices, const int* data, const u64* ww,
                                                 const double* phi, u32 n_haps, double* r, u64* parts) {
    __shared__ double v[Q_TILE];
    __shared__ u64 s[TPB];
    if (st->done) return;
    const u64 e0 = blockIdx.x * (u64)TPB, e = e0 + threadIdx.x;
    const u32 lo = (u32)indptr[e0], hi = (u32)indptr[std::min<u64>(n_ecs, e0 + TPB)];
    u32 a = 0, b = 0;
    if (e < n_ecs) { a = (u32)indptr[e]; b = (u32)indptr[e + 1]; }
    const bool mine = e < n_ecs && b - a <= Q_LONG_ROW;
    const double d = q_tile_pass<Q_TILE>(v, phi, n_haps, indices, data, lo, hi, a, b, mine);
    u64 got = 0;
    if (mine) q_row_done(ww[e], d, r + e, got);
    got = q_block_sum(got, s);
    if (threadIdx.x == 0) parts[blockIdx.x] = got;
}
// E-step, workgroup b: long row long_rows[b] -- thread k sums non-zeros k, k + TPB, ... in that order, the tree folds the TPB sums
__global__ __launch_bounds__(TPB) void k_q_elong(const QState* st, const u32* long_rows, const int* indptr, const int* indices, const int* data,
                                                 const u64* ww, const double* phi, u32 n_haps, double* r, u64* parts) {
    __shared__ double s[TPB];
    if (st->done) return;
    const u32 e = long_rows[blockIdx.x];
    const double d = q_long_row_sum(s, phi, n_haps, indices, data, (u32)indptr[e], (u32)indptr[e + 1]);
    if (threadIdx.x == 0) {
        u64 got;
        q_row_done(ww[e], d, r + e, got);
        parts[blockIdx.x] = got;
    }
}
// The long-column fold of the M-step (k_q_mlong, k_qc_mlong; k_qm_mlong, k_qcm_mlong).  Column [a, b) of the column view is read once for
// all its haplotypes, TPB entries at a time: thread k puts entry k's mask and what `load` gives for it into LDS (its row's r or weight: one
// gather per entry, not one per set bit; or where its coefficients start); then, with haplotype h = k % hp (hp: the power of two at or above
// H), it adds term(x, mask, h) of the entries k / hp, k / hp + TPB / hp, ... with its bit.  The tree folds the TPB / hp sums of a haplotype:
// thread h < hp gets the column's sum for h (every thread of the workgroup calls this)
template <class V, class X, class M, class Load, class Term>
__device__ __forceinline__ V q_col_fold(V* s, X* x, u32* msk, const M* col_mask, u32 a, u32 b, u32 hp, Load load, Term term) {
    const u32 h = threadIdx.x & (hp - 1u), slot = threadIdx.x / hp, stride = TPB / hp;
    V acc = 0;
    for (u32 base = a; base < b; base += TPB) {
        const u32 n = std::min<u32>(TPB, b - base);
        if (threadIdx.x < n) {
            msk[threadIdx.x] = (u32)col_mask[base + threadIdx.x];
            x[threadIdx.x] = load(base + threadIdx.x);
        }
        __syncthreads();
        for (u32 j = slot; j < n; j += stride)
            if ((msk[j] >> h) & 1u) acc += term(x[j], msk[j], h);
        __syncthreads();
    }
    return q_block_sum(acc, s, hp);
}
// M-step, workgroup b: long column long_cols[b] -- q_col_fold over its entries' r; the sums go to acc_long[t H + h] for k_q_mstep to use.
// INIT: the sums of the weights instead (theta_0 = aln), exact in 64-bit integers
template <bool INIT>
__global__ __launch_bounds__(TPB) void k_q_mlong(const QState* st, const u32* long_cols, const int* colptr, const int* col_ec, const int* col_mask,
                                                 const double* r, const u64* ww, u32 n_haps, u32 hp, double* acc_long) {
    using V = typename std::conditional<INIT, u64, double>::type;
    __shared__ V s[TPB], val[TPB];
    __shared__ u32 msk[TPB];
    if (!INIT && st->done) return;
    const u32 t = long_cols[blockIdx.x];
    const V acc = q_col_fold(s, val, msk, col_mask, (u32)colptr[t], (u32)colptr[t + 1], hp,
                             [&](u32 k) { if constexpr (INIT) return (V)ww[col_ec[k]]; else return (V)r[col_ec[k]]; }, [](V x, u32, u32) { return x; });
    if (threadIdx.x < n_haps) acc_long[(u64)t * n_haps + threadIdx.x] = (double)acc;
}
// item i of an M-step: theta' = phi x the column's sum (INIT: the sum itself), the next phi; |theta' - theta| back (INIT: unused)
template <bool INIT> __device__ __forceinline__ double q_theta_next(double acc, u64 i, const double* scale, double* theta, double* phi) {
    const double was = INIT ? 0.0 : theta[i], now = INIT ? acc : phi[i] * acc;
    theta[i] = now;
    phi[i] = scale ? now * scale[i] : now;
    return fabs(now - was);
}
// M-step, thread i = t H + h: the entries of column t with bit h, in index order (ascending EC); theta', the next phi, and the workgroup's
// part of delta.  INIT: theta_0 = aln, no delta
template <bool INIT>
__global__ __launch_bounds__(TPB) void k_q_mstep(const QState* st, const int* colptr, const int* col_ec, const int* col_mask, const double* r,
                                                 const u64* ww, const double* acc_long, const double* scale, u32 n_loci, u32 n_haps, double* theta,
                                                 double* phi, double* partial) {
    __shared__ double s[TPB];
    if (!INIT && st->done) return;
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    double diff = 0.0;
    if (i < (u64)n_loci * n_haps) {
        const u32 t = (u32)(i / n_haps), h = (u32)(i - (u64)t * n_haps);
        const u32 a = (u32)colptr[t], b = (u32)colptr[t + 1];
        double acc;
        if (b - a > Q_LONG_COL) acc = acc_long[i];
        else if (INIT) {
            u64 n = 0;
            for (u32 k = a; k < b; ++k)
                if (((u32)col_mask[k] >> h) & 1u) n += ww[col_ec[k]];
            acc = (double)n;
        } else {
            acc = 0.0;
            for (u32 k = a; k < b; ++k)
                if (((u32)col_mask[k] >> h) & 1u) acc += r[col_ec[k]];
        }
        diff = q_theta_next<INIT>(acc, i, scale, theta, phi);
    }
    if (INIT) return;
    diff = q_block_sum(diff, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = diff;
}
// one workgroup: delta = the parts in a fixed order (thread k: parts k, k + TPB, ...; then the tree), the explained reads likewise; the step
// counted, the stop decided
__global__ __launch_bounds__(TPB) void k_q_conv(QState* st, const double* partial, u32 n_parts, const u64* expl_parts, u32 n_expl) {
    __shared__ double s[TPB];
    __shared__ u64 sw[TPB];
    if (st->done) return;
    const u64 explained = q_parts_sum(expl_parts, n_expl, sw);
    double d = 0.0;
    for (u32 k = threadIdx.x; k < n_parts; k += TPB) d += partial[k];
    d = q_block_sum(d, s);
    if (threadIdx.x != 0) return;
    st->delta = d;
    st->n_iter += 1u;
    st->explained = explained;
    if (d <= st->stop) { st->converged = 1u; st->done = 1u; }
    else if (st->n_iter >= st->max_iters) st->done = 1u;
}
// theta T x H -> the caller's H x T
__global__ __launch_bounds__(TPB) void k_q_out(const double* theta, u32 n_loci, u32 n_haps, double* out) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= (u64)n_loci * n_haps) return;
    const u32 h = (u32)(i / n_loci), t = (u32)(i - (u64)h * n_loci);
    out[i] = theta[(u64)t * n_haps + h];
}

// ---- the host side every ecquant entry point shares: the matrices, the validation front, the sort buffers, the column view, the driver ----
// A, and N when there is one (pn null: the posterior has none), as device or as host arrays
struct QMat {
    u32 n_ecs, n_loci, n_haps; u64 nnz; const int *ip, *ix, *da;
    u32 n_samples; u64 nnz_n; const int *pn, *xn, *dn;
};
struct QModel { u32 model, n_genes; const int* gene; };              // a hierarchical model over a gene grouping (nullptr: the flat step)
// the four scalars of a run, and their way to the caller
struct QResult {
    uint32_t n_iter = 0; double delta = 0.0; int64_t explained = 0; uint32_t converged = 0;
    void put(uint32_t* it, double* dl, int64_t* ex, uint32_t* cv) const {
        if (it) *it = n_iter;
        if (dl) *dl = delta;
        if (ex) *ex = explained;
        if (cv) *cv = converged;
    }
};
// what the flat and the model entry points refuse before anything is allocated (count-alignments' refusals, then ecquant's own)
int q_check_args(const QMat& m, int64_t sample, double tol, const void* theta) {
    RCCHK(ca_check_matrices(m.n_ecs, m.n_loci, m.n_haps, m.nnz, m.ip, m.ix, m.da, m.n_samples, m.nnz_n, m.pn, m.xn, m.dn));
    if (!theta || !(tol >= 0.0)) return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no theta, or a tolerance that is NaN or negative)");
    if (m.nnz >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: 2^30 non-zeros or more");       // (radix_sort_pairs64)
    if ((u64)m.n_haps * m.n_loci >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x loci does not fit 31 bits");
    if (sample < -1 || sample >= (int64_t)m.n_samples)
        return fail(nullptr, ECB_ERR_CONTRACT, "ecquant: no such sample (%lld of %u)", (long long)sample, m.n_samples);
    return ECB_OK;
}

// The validation front.  A checked and its set bits counted and scanned (bits_excl: nnz + 1 values), the weights of N's column `sample`
// (-1: all of them) when there is an N, the caller's tables checked and brought T x H into the call's own buffers, the gene ids checked
// (with_keys: and the keys of the members' CSR left in gk[0] / gv[0]); one read-back, then the refusals in their order: A, N, the set-bit
// limit, `errs`.  Nothing of the caller's is written.  own_tables: theta and phi are the call's state whether or not a theta comes in.
struct QFront {
    u64* words;                      // apply-mask's words; [1] the error bits of N, [3] the set bits, [4] the sort's, [5] the error bits of the tables and of gene
    u32 *bits_excl, *sums;           // (sums: scan scratch for n_scan values)
    u64* ww;
    double *theta, *phi, *scale;     // T x H
    u64* gk[2]; u32* gv[2];
    u64 n_bits;
    std::vector<u64> back;
};
__global__ __launch_bounds__(TPB) void k_qm_gkeys(const int* gene, u32 n_loci, u32 n_genes, u64* keys, u32* vals, u32* err);          // (quant_model.inc)
int q_front(Call& c, const QMat& m, int64_t sample, const void* d_scale, const void* d_theta, u32 theta_bit, bool own_tables, const int* gene,
            u32 n_genes, bool with_keys, u64 n_scan, const ErrBit (&errs)[3], QFront& f) {
    hipStream_t st = c.st;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS), n_tab = (u64)m.n_haps * m.n_loci, nnz = m.nnz;
    f = QFront{};
    f.words = c.get<u64>(CV_WORDS, n_words);
    u32* bits = c.get<u32>(CV_X0, nnz);
    f.bits_excl = c.get<u32>(CV_X1, nnz + 1); f.sums = c.get<u32>(CV_SUMS2, scan_words(n_scan));
    if (m.pn) f.ww = c.get<u64>(CV_X2, m.n_ecs);
    if (own_tables || d_theta) f.theta = c.get<double>(n_tab);
    if (own_tables) f.phi = c.get<double>(n_tab);
    if (d_scale) f.scale = c.get<double>(n_tab);
    if (with_keys) { f.gk[0] = c.get<u64>(m.n_loci); f.gk[1] = c.get<u64>(m.n_loci); f.gv[0] = c.get<u32>(m.n_loci); f.gv[1] = c.get<u32>(m.n_loci); }
    if (const int rc = c.missing()) return rc;
    u32* err = reinterpret_cast<u32*>(f.words + 5);
    CALLCHK(c, hipMemsetAsync(f.words, 0, n_words * 8, st));
    if (m.pn) {
        CALLCHK(c, hipMemsetAsync(f.ww, 0, std::max<u64>(m.n_ecs, 1) * 8, st));
        k_ca_weights<<<nblk(std::max<u64>(m.nnz_n, (u64)m.n_samples + 1), TPB), TPB, 0, st>>>(m.pn, m.n_samples, m.xn, m.dn, m.nnz_n, m.n_ecs, sample, f.ww,
                                                                                             f.words);
    }
    k_gm_check<true><<<nblk(std::max<u64>((u64)m.n_ecs + 1, (nnz + GM_ITEMS - 1) / GM_ITEMS), TPB), TPB, 0, st>>>(m.ip, m.n_ecs, m.ix, m.da, nnz, nullptr,
                                                                                                               m.n_loci, m.n_haps, bits, f.words);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, bits, nnz, f.bits_excl, f.sums, f.words + 3, 1, f.bits_excl + nnz));
    // (into the call's own tables, T x H: nothing of the caller's is written yet)
    if (d_scale) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_scale, m.n_loci, m.n_haps, f.scale, Q_ERR_SCALE, err);
    if (d_theta) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_theta, m.n_loci, m.n_haps, f.theta, theta_bit, err);
    if (gene && m.n_loci) k_qm_gkeys<<<nblk(m.n_loci, TPB), TPB, 0, st>>>(gene, m.n_loci, n_genes, f.gk[0], f.gv[0], err);
    CALLCHK(c, hipGetLastError());
    f.back.resize(n_words);
    if (const int rc = c.read_back(f.back.data(), f.words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(f.back));
    if (f.back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");      // (as count-alignments: bits_excl is 32 bits wide)
    RCCHK(refuse_bits(nullptr, errs, (u32)f.back[5]));
    f.n_bits = f.back[3];
    return ECB_OK;
}

// the pool's buffers for sorts of up to n pairs (n_hist: the longest sort they serve, when that is another's); the caller asks c.missing()
struct QSort { SortBufs s; SortScratch ss; };
QSort q_sort_bufs(Call& c, u64 n, u64 n_hist, u64* d_word) {
    u64 *k0 = c.get<u64>(CV_KEYS0, n), *k1 = c.get<u64>(CV_KEYS1, n);
    u32 *v0 = c.get<u32>(CV_VALS0, n), *v1 = c.get<u32>(CV_VALS1, n);
    return QSort{SortBufs{{k0, k1}, {v0, v1}}, SortScratch{c.get<u32>(CV_HIST, rs_words(n_hist)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), d_word}};
}

// The column view: the non-zeros sorted by locus, stable, so the ECs of a column ascend.  with_b0 (the models): and where the coefficients
// of each entry's non-zero start.  srt's buffers are free again afterwards
struct QCols { int *colptr, *col_ec, *col_mask; u32* col_b0; };
__global__ __launch_bounds__(TPB) void k_qm_colbase(const u64* ckeys, u64 nnz, const int* indptr, const int* indices, const u32* bits_excl, u32* col_b0);      // (quant_model.inc)
int q_col_view(Call& c, const QMat& m, const QFront& f, QSort& srt, bool with_b0, QCols& v) {
    hipStream_t st = c.st;
    const u64 nnz = m.nnz;
    v = QCols{c.get<int>((u64)m.n_loci + 1), c.get<int>(nnz), c.get<int>(nnz), with_b0 ? c.get<u32>(nnz) : nullptr};
    if (const int rc = c.missing()) return rc;
    k_cv_keys<<<nblk(m.n_ecs, TPB), TPB, 0, st>>>(m.ip, m.n_ecs, m.ix, m.da, nnz, m.n_loci, m.n_haps, srt.s.k[0], srt.s.v[0],
                                                 reinterpret_cast<u32*>(f.words + 6));      // (its verdict is not read: a mask of 0 is allowed here)
    CALLCHK(c, radix_sort_pairs64(st, srt.s, nnz, srt.ss, msb_mask(m.n_loci - 1) << 32));
    k_split_out<<<nblk(nnz, TPB), TPB, 0, st>>>(srt.s.keys(), srt.s.vals(), nnz, v.col_ec, v.col_mask);
    k_row_ptr<<<nblk((u64)m.n_loci + 1, TPB), TPB, 0, st>>>(srt.s.keys(), nnz, m.n_loci, v.colptr);
    if (with_b0) k_qm_colbase<<<nblk(nnz, TPB), TPB, 0, st>>>(srt.s.keys(), nnz, m.ip, m.ix, f.bits_excl, v.col_b0);
    CALLCHK(c, hipGetLastError());
    return ECB_OK;
}

// The hierarchical models (quant_model.inc, included after this file) run on a call as q_run set it up: what it hands them (QView), what
// they add to the set-up (QmTabs: the gene view and the chain's tables) and their step in place of the E- and M-step kernels.  The
// posterior (quant_post.inc) runs the same chain once, with `post` set: k_qp_post then takes the place of the coefficients and the M-step.
struct QView {
    hipStream_t st;
    u32 n_ecs, n_loci, n_haps, hp, n_eblk, n_parts, nlr, nlc; u64 nnz;
    const int *ip, *ix, *da;
    const u32 *bits_excl, *long_rows, *long_cols;
    QCols cols;
    const u64* ww;
    const QState* qs;
    const double* scale;
    double *theta, *phi, *acc_long, *partial;
    u64* expl_parts;                 // the short rows' workgroups, then the long rows'
};
struct QGenes {
    u32 n_genes;
    int *gptr, *gmem; u32* long_genes;                                 // the members of each gene as a CSR (loci ascending), the genes above Q_LONG_GENE
    const u64* rkeys; const u32* gnz;                                  // the gene-ordered view of the rows: (row, gene) and non-zero of every position
    u32 *segid, *seg_start, *nz_seg;                                   // its segments
    u64* cnt;                                                          // on the device: [0] the segments, [1] the long genes; the caller reads them back ...
    u32 n_segs, n_long_genes;                                          // ... into these, with a wait it has anyway
};
struct QmTabs { QGenes g; double *phi_gh, *phi_g, *phi_t, *seg_c, *seg_x, *coef; };
int qm_check_genes(int device, const char* prefix, const int* gene, u32 n_loci, u32 n_genes);
int qm_setup(Call& c, const QMat& m, const QFront& f, const QModel& mdl, QSort& srt, QmTabs& t);
void qm_step(const QView& v, const QmTabs& t, u32 model, bool post);

// Both device entry points, their arguments checked.  mdl = nullptr: the flat step, this file's own; model 4 is that step too, the genes
// checked first in a call of their own.
int q_run(int device, const QMat& m, int64_t sample, const void* d_scale, const void* d_theta_in, u32 max_iters, double tol, void* d_theta,
          QResult& res, const QModel* mdl = nullptr) {
    if (mdl && mdl->model == 4u) {
        RCCHK(qm_check_genes(device, "ecquant: ", mdl->gene, m.n_loci, mdl->n_genes));
        mdl = nullptr;
    }
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u32 n_ecs = m.n_ecs, n_loci = m.n_loci, n_haps = m.n_haps;
    const u64 nnz = m.nnz, n_tab = (u64)n_haps * n_loci;
    QFront f;
    RCCHK(q_front(c, m, sample, d_scale, d_theta_in, Q_ERR_THETA, true, mdl ? mdl->gene : nullptr, mdl ? mdl->n_genes : 0u, mdl != nullptr,
                  mdl ? nnz + 1 : nnz, Q_ERRS, f));
    // the input is well formed: from here on the outputs are written
    QState fin{};
    fin.converged = 1u;
    if (!n_ecs || !nnz) CALLCHK(c, hipMemsetAsync(d_theta, 0, n_tab * 8, st));
    else {
        QSort srt = q_sort_bufs(c, nnz, mdl ? std::max<u64>(nnz, n_loci) : nnz, f.words + 4);
        u32 *long_rows = c.get<u32>(nnz / Q_LONG_ROW + 1), *long_cols = c.get<u32>(nnz / Q_LONG_COL + 1);
        const u32 n_parts = nblk(n_tab, TPB);
        const u32 n_eblk = nblk(n_ecs, TPB);
        double *r = mdl ? nullptr : c.get<double>(n_ecs), *acc_long = c.get<double>(n_tab), *partial = c.get<double>(n_parts);
        u64* expl_parts = c.get<u64>((u64)n_eblk + nnz / Q_LONG_ROW + 1);
        QState* qs = c.get<QState>(1);
        if (const int rc = c.missing()) return rc;
        CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QState), st));
        QCols cv;
        RCCHK(q_col_view(c, m, f, srt, mdl != nullptr, cv));
        QmTabs mt{};
        if (mdl) RCCHK(qm_setup(c, m, f, *mdl, srt, mt));          // (after the column view: the gene-ordered view stays in srt's buffers)
        const int *colptr = cv.colptr, *col_ec = cv.col_ec, *col_mask = cv.col_mask;
        k_q_rows<<<n_eblk, TPB, 0, st>>>(m.ip, n_ecs, f.bits_excl, f.ww, qs, long_rows, expl_parts);
        k_q_w<<<1, TPB, 0, st>>>(qs, expl_parts, n_eblk);
        k_q_cols<<<nblk(n_loci, TPB), TPB, 0, st>>>(colptr, n_loci, qs, long_cols);
        CALLCHK(c, hipGetLastError());
        QState q0;
        u64 gcnt[2] = {0, 0};
        CALLCHK(c, hipMemcpyAsync(&q0, qs, sizeof(QState), hipMemcpyDeviceToHost, st));
        if (mdl) CALLCHK(c, hipMemcpyAsync(gcnt, mt.g.cnt, 16, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
        mt.g.n_segs = (u32)gcnt[0]; mt.g.n_long_genes = (u32)gcnt[1];
        const u32 nlr = q0.n_long_rows, nlc = q0.n_long_cols;
        u32 hp = 1;
        while (hp < n_haps) hp <<= 1;
        double *theta = f.theta, *phi = f.phi;
        const double* scale = f.scale;
        const u64* ww = f.ww;
        const QView view{st, n_ecs, n_loci, n_haps, hp, n_eblk, n_parts, nlr, nlc, nnz, m.ip, m.ix, m.da, f.bits_excl, long_rows, long_cols, cv, ww, qs,
                         scale, theta, phi, acc_long, partial, expl_parts};
        k_q_arm<<<1, 1, 0, st>>>(qs, max_iters, tol * (double)q0.W);
        if (d_theta_in) k_q_phi<<<nblk(n_tab, TPB), TPB, 0, st>>>(theta, scale, n_tab, phi);
        else {
            if (nlc) k_q_mlong<true><<<nlc, TPB, 0, st>>>(qs, long_cols, colptr, col_ec, col_mask, r, ww, n_haps, hp, acc_long);
            k_q_mstep<true><<<n_parts, TPB, 0, st>>>(qs, colptr, col_ec, col_mask, r, ww, acc_long, scale, n_loci, n_haps, theta, phi, partial);
        }
        CALLCHK(c, hipGetLastError());
        fin = QState{};
        fin.done = max_iters == 0u;
        for (u32 queued = 0; !fin.done;) {
            for (u32 k = 0; k < Q_BATCH && queued < max_iters; ++k, ++queued) {
                if (mdl) qm_step(view, mt, mdl->model, false);
                else {
                    if (nlr) k_q_elong<<<nlr, TPB, 0, st>>>(qs, long_rows, m.ip, m.ix, m.da, ww, phi, n_haps, r, expl_parts + n_eblk);
                    k_q_estep<<<n_eblk, TPB, 0, st>>>(qs, m.ip, n_ecs, m.ix, m.da, ww, phi, n_haps, r, expl_parts);
                    if (nlc) k_q_mlong<false><<<nlc, TPB, 0, st>>>(qs, long_cols, colptr, col_ec, col_mask, r, ww, n_haps, hp, acc_long);
                    k_q_mstep<false><<<n_parts, TPB, 0, st>>>(qs, colptr, col_ec, col_mask, r, ww, acc_long, scale, n_loci, n_haps, theta, phi, partial);
                }
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
    res = QResult{fin.n_iter, fin.delta, (int64_t)fin.explained, fin.converged};
    return ECB_OK;
}

// A, and N when there is one, on their way to the device: the head of a host entry point's StageIn list
struct QStage { DevBuf<> ipa, ixa, daa, ipn, ixn, dan; };
std::vector<StageIn> q_stage(QStage& b, const QMat& m) {
    std::vector<StageIn> in = {{&b.ipa, m.ip, ((u64)m.n_ecs + 1) * 4}, {&b.ixa, m.ix, m.nnz * 4}, {&b.daa, m.da, m.nnz * 4}};
    if (m.pn) in.insert(in.end(), {{&b.ipn, m.pn, ((u64)m.n_samples + 1) * 4}, {&b.ixn, m.xn, m.nnz_n * 4}, {&b.dan, m.dn, m.nnz_n * 4}});
    return in;
}
// ... and the same matrices where they then are
QMat q_staged(const QStage& b, const QMat& m) {
    return QMat{m.n_ecs, m.n_loci, m.n_haps, m.nnz, b.ipa.as<int>(), b.ixa.as<int>(), b.daa.as<int>(),
                m.n_samples, m.nnz_n, b.ipn.as<int>(), b.ixn.as<int>(), b.dan.as<int>()};
}
// Both host entry points, their arguments checked: everything staged, the device run, theta and the scalars back
int q_host(int device, const QMat& m, int64_t sample, const double* scale, const double* theta_in, u32 max_iters, double tol, const QModel* mdl,
           double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    const u64 plane = (u64)m.n_haps * m.n_loci * 8;
    QStage b;
    DevBuf<> sc, ti, gn, out;
    std::vector<StageIn> in = q_stage(b, m);
    if (mdl) in.push_back({&gn, mdl->gene, (u64)m.n_loci * 4});
    in.push_back({&out, nullptr, plane});
    if (scale) in.push_back({&sc, scale, plane});
    if (theta_in) in.push_back({&ti, theta_in, plane});
    RCCHK(stage_in(c, in));
    const QModel dm{mdl ? mdl->model : 4u, mdl ? mdl->n_genes : 0u, gn.as<int>()};
    QResult res;
    RCCHK(q_run(device, q_staged(b, m), sample, sc.p, ti.p, max_iters, tol, out.p, res, mdl ? &dm : nullptr));
    RCCHK(stage_out(c, {{theta, &out, plane}}));
    res.put(n_iter, delta, explained, converged);
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_quantify_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                   const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                   const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                                   uint32_t max_iters, double tol, void* d_theta, uint32_t* n_iter, double* delta, int64_t* explained,
                                   uint32_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(q_check_args(m, sample, tol, d_theta));
    QResult res;
    RCCHK(q_run(device, m, sample, d_scale, d_theta_in, max_iters, tol, d_theta, res));
    res.put(n_iter, delta, explained, converged);
    return ECB_OK;
}

extern "C" int ecb_quantify(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                            const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                            const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                            uint32_t max_iters, double tol, double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(q_check_args(m, sample, tol, theta));
    return q_host(device, m, sample, scale, theta_in, max_iters, tol, nullptr, theta, n_iter, delta, explained, converged);
}
