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
namespace {
constexpr u32 Q_LONG_ROW = 256;      // a row with more non-zeros than this is summed by a workgroup, not a lane
constexpr u32 Q_LONG_COL = 32;       // a column with more entries than this likewise (its lane would wait for every entry in turn: 256 cost 0.2 ms)
constexpr u32 Q_TILE = 2048;        // k_q_estep: non-zeros of a workgroup's rows in LDS at a time
constexpr u32 Q_BATCH = 8;           // steps enqueued between two looks at the device's state
enum : u32 { Q_ERR_SCALE = 1u, Q_ERR_THETA = 2u };
struct QState {
    u32 done, n_iter, converged, max_iters;
    double delta, stop;              // stop = tol x W
    u64 explained, W;                // of the last whole step; of the matrix
    u32 n_long_rows, n_long_cols;
};
const ErrBit Q_ERRS[] = {
    {Q_ERR_SCALE, ECB_ERR_CONTRACT, "ecquant: an entry of scale is NaN, infinite or negative"},
    {Q_ERR_THETA, ECB_ERR_CONTRACT, "ecquant: an entry of theta_in is NaN, infinite or negative"},
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
// E-step, the short rows.  Workgroup b has rows [b TPB, (b + 1) TPB), whose non-zeros are one stretch of A: it goes through LDS Q_TILE
// non-zeros at a time -- thread k the phi of non-zeros k, k + TPB, ... of the tile (its set bits, lowest first: coalesced loads, the same work
// for every lane whatever the rows' lengths), then lane e adds those of row e in index order.  parts[b] = the weights the workgroup explained.
// The non-zeros of a long row in the stretch are staged like the others and then read by nobody (k_q_elong has summed them): wasted
// gathers, one tile per Q_TILE of them -- 94 k of config 3's 13 M non-zeros; tiles that lie inside a long row are not skipped.
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
    double d = 0.0;
    for (u32 base = lo; base < hi; base += Q_TILE) {
        const u32 n = std::min<u32>(Q_TILE, hi - base);
        for (u32 k = threadIdx.x; k < n; k += TPB) v[k] = q_bits_sum(phi, n_haps, (u32)indices[base + k], (u32)data[base + k], 0.0);
        __syncthreads();
        if (mine)
            for (u32 i = std::max(a, base), y = std::min(b, base + n); i < y; ++i) d += v[i - base];
        __syncthreads();
    }
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
    const u32 a = (u32)indptr[e], b = (u32)indptr[e + 1];
    double d = 0.0;
    for (u32 i = a + threadIdx.x; i < b; i += TPB) d = q_bits_sum(phi, n_haps, (u32)indices[i], (u32)data[i], d);
    d = q_block_sum(d, s);
    if (threadIdx.x == 0) {
        u64 got;
        q_row_done(ww[e], d, r + e, got);
        parts[blockIdx.x] = got;
    }
}
// M-step, workgroup b: long column long_cols[b], read once for all its haplotypes, TPB entries at a time: thread k puts entry k's mask and
// its row's r (one gather per entry, not one per set bit) into LDS; then, with haplotype k % hp (hp: the power of two at or above H), it adds
// of the entries k / hp, k / hp + TPB / hp, ... those with its bit.  The tree folds the TPB / hp sums of a haplotype; they go to
// acc_long[t H + h] for k_q_mstep to use.  INIT: the sums of the weights instead (theta_0 = aln), exact in 64-bit integers
template <bool INIT>
__global__ __launch_bounds__(TPB) void k_q_mlong(const QState* st, const u32* long_cols, const int* colptr, const int* col_ec, const int* col_mask,
                                                 const double* r, const u64* ww, u32 n_haps, u32 hp, double* acc_long) {
    using V = typename std::conditional<INIT, u64, double>::type;
    __shared__ V s[TPB], val[TPB];
    __shared__ u32 msk[TPB];
    if (!INIT && st->done) return;
    const u32 t = long_cols[blockIdx.x], h = threadIdx.x & (hp - 1u), slot = threadIdx.x / hp, stride = TPB / hp;
    const u32 a = (u32)colptr[t], b = (u32)colptr[t + 1];
    V acc = 0;
    for (u32 base = a; base < b; base += TPB) {
        const u32 n = std::min<u32>(TPB, b - base);
        if (threadIdx.x < n) {
            msk[threadIdx.x] = (u32)col_mask[base + threadIdx.x];
            if (INIT) val[threadIdx.x] = (V)ww[col_ec[base + threadIdx.x]];
            else val[threadIdx.x] = (V)r[col_ec[base + threadIdx.x]];
        }
        __syncthreads();
        for (u32 j = slot; j < n; j += stride)
            if ((msk[j] >> h) & 1u) acc += val[j];
        __syncthreads();
    }
    acc = q_block_sum(acc, s, hp);
    if (threadIdx.x < n_haps) acc_long[(u64)t * n_haps + threadIdx.x] = (double)acc;
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
        const double was = INIT ? 0.0 : theta[i], now = INIT ? acc : phi[i] * acc;
        theta[i] = now;
        phi[i] = scale ? now * scale[i] : now;
        diff = fabs(now - was);
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
// what both entry points refuse before anything is allocated (count-alignments' refusals, then ecquant's own)
int q_check_args(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* indptr_a, const void* indices_a, const void* data_a,
                 uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int64_t sample, double tol,
                 const void* theta) {
    RCCHK(ca_check_matrices(n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n));
    if (!theta || !(tol >= 0.0)) return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no theta, or a tolerance that is NaN or negative)");
    if (nnz_a >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: 2^30 non-zeros or more");       // (radix_sort_pairs64)
    if ((u64)n_haps * n_loci >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x loci does not fit 31 bits");
    if (sample < -1 || sample >= (int64_t)n_samples) return fail(nullptr, ECB_ERR_CONTRACT, "ecquant: no such sample (%lld of %u)", (long long)sample, n_samples);
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_quantify_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                   const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                   const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, const void* d_theta_in,
                                   uint32_t max_iters, double tol, void* d_theta, uint32_t* n_iter, double* delta, int64_t* explained,
                                   uint32_t* converged) {
    RCCHK(q_check_args(n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, sample, tol,
                       d_theta));
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);          // apply-mask's words; [1] the error bits of N, [5] those of scale and theta_in
    const u64 n_tab = (u64)n_haps * n_loci;
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *bits = c.get<u32>(CV_X0, nnz), *bits_excl = c.get<u32>(CV_X1, nnz + 1), *sums = c.get<u32>(CV_SUMS2, scan_words(nnz));
    u64* ww = c.get<u64>(CV_X2, n_ecs);
    double *theta = c.get<double>(n_tab), *phi = c.get<double>(n_tab), *scale = d_scale ? c.get<double>(n_tab) : nullptr;
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
    // (into the call's own tables, T x H: nothing of the caller's is written yet)
    if (d_scale) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_scale, n_loci, n_haps, scale, Q_ERR_SCALE, reinterpret_cast<u32*>(words + 5));
    if (d_theta_in) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_theta_in, n_loci, n_haps, theta, Q_ERR_THETA, reinterpret_cast<u32*>(words + 5));
    CALLCHK(c, hipGetLastError());
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    if (back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");      // (as count-alignments: bits_excl is 32 bits wide)
    RCCHK(refuse_bits(nullptr, Q_ERRS, (u32)back[5]));
    // the input is well formed: from here on the outputs are written
    QState fin{};
    fin.converged = 1u;
    if (!n_ecs || !nnz) CALLCHK(c, hipMemsetAsync(d_theta, 0, n_tab * 8, st));
    else {
        // the column view: the non-zeros sorted by locus, ECs ascending within a column
        u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
        u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
        SortScratch ss{c.get<u32>(CV_HIST, rs_words(nnz)), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 4};
        int *colptr = c.get<int>((u64)n_loci + 1), *col_ec = c.get<int>(nnz), *col_mask = c.get<int>(nnz);
        u32 *long_rows = c.get<u32>(nnz / Q_LONG_ROW + 1), *long_cols = c.get<u32>(nnz / Q_LONG_COL + 1);
        const u32 n_parts = nblk(n_tab, TPB);
        const u32 n_eblk = nblk(n_ecs, TPB);
        double *r = c.get<double>(n_ecs), *acc_long = c.get<double>(n_tab), *partial = c.get<double>(n_parts);
        u64* expl_parts = c.get<u64>((u64)n_eblk + nnz / Q_LONG_ROW + 1);          // the short rows' workgroups, then the long rows' 
        QState* qs = c.get<QState>(1);
        if (const int rc = c.missing()) return rc;
        CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QState), st));
        k_cv_keys<<<nblk(n_ecs, TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, n_loci, n_haps, k0, v0, reinterpret_cast<u32*>(words + 6));   // (its verdict is not read: a mask of 0 is allowed here)
        SortBufs s{{k0, k1}, {v0, v1}};
        CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_loci - 1) << 32));
        k_split_out<<<nblk(nnz, TPB), TPB, 0, st>>>(s.keys(), s.vals(), nnz, col_ec, col_mask);
        k_row_ptr<<<nblk((u64)n_loci + 1, TPB), TPB, 0, st>>>(s.keys(), nnz, n_loci, colptr);
        k_q_rows<<<n_eblk, TPB, 0, st>>>(ip, n_ecs, bits_excl, ww, qs, long_rows, expl_parts);
        k_q_w<<<1, TPB, 0, st>>>(qs, expl_parts, n_eblk);
        k_q_cols<<<nblk(n_loci, TPB), TPB, 0, st>>>(colptr, n_loci, qs, long_cols);
        CALLCHK(c, hipGetLastError());
        QState q0;
        CALLCHK(c, hipMemcpyAsync(&q0, qs, sizeof(QState), hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
        const u32 nlr = q0.n_long_rows, nlc = q0.n_long_cols;
        u32 hp = 1;
        while (hp < n_haps) hp <<= 1;
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
                if (nlr) k_q_elong<<<nlr, TPB, 0, st>>>(qs, long_rows, ip, ix, da, ww, phi, n_haps, r, expl_parts + n_eblk);
                k_q_estep<<<n_eblk, TPB, 0, st>>>(qs, ip, n_ecs, ix, da, ww, phi, n_haps, r, expl_parts);
                if (nlc) k_q_mlong<false><<<nlc, TPB, 0, st>>>(qs, long_cols, colptr, col_ec, col_mask, r, ww, n_haps, hp, acc_long);
                k_q_mstep<false><<<n_parts, TPB, 0, st>>>(qs, colptr, col_ec, col_mask, r, ww, acc_long, scale, n_loci, n_haps, theta, phi, partial);
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

extern "C" int ecb_quantify(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                            const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                            const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, const double* theta_in,
                            uint32_t max_iters, double tol, double* theta, uint32_t* n_iter, double* delta, int64_t* explained, uint32_t* converged) {
    RCCHK(q_check_args(n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n, sample, tol, theta));
    Call c(device, "ecquant: "); if (c.rc) return c.rc;
    const u64 plane = (u64)n_haps * n_loci * 8;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, sc, ti, out;
    std::vector<StageIn> in = {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz * 4}, {&daa, data_a, nnz * 4},
                               {&ipn, indptr_n, ((u64)n_samples + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4},
                               {&out, nullptr, plane}};
    if (scale) in.push_back({&sc, scale, plane});
    if (theta_in) in.push_back({&ti, theta_in, plane});
    int rc = stage_in(c, in);
    uint32_t it = 0, conv = 0; double dl = 0.0; int64_t ex = 0;
    if (rc == ECB_OK) rc = ecb_quantify_device(device, n_ecs, n_loci, n_haps, nnz, ipa.p, ixa.p, daa.p, n_samples, nnz_n, ipn.p, ixn.p, dan.p, sample,
                                               sc.p, ti.p, max_iters, tol, out.p, &it, &dl, &ex, &conv);
    RCCHK(rc);
    RCCHK(stage_out(c, {{theta, &out, plane}}));
    if (n_iter) *n_iter = it;
    if (delta) *delta = dl;
    if (explained) *explained = ex;
    if (converged) *converged = conv;
    return ECB_OK;
}
