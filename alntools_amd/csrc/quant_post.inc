// ---- ecquant's posterior: one probability per set bit of A at a given theta (ecb_posterior / ecb_posterior_device; included by ecb.hip after
// quant_model.inc) -- what the E-step forms and throws away (r[e] in k_q_estep, a coefficient per set bit in k_qm_coef), kept.
// (AlignmentPropertyMatrix.multiply(axis=2) / normalize_reads(axis=READ | HAPLOGROUP | LOCUS | GROUP), AlignmentPropertyMatrix.py:219-384, without
//  the sum over reads; what AlignmentPropertyMatrix.save(incidence_only=False) stores.)
// The values go out in BIT ORDER: the non-zeros in storage order, the set bits of one lowest first -- the place bits_excl[i] + the set bits
// below h, as the models' coefficients are laid out.  No weights: a row's posterior does not depend on its count.
// Flat model: the row pass of ecquant with the sum itself kept (k_qp_dlong: a workgroup per long row; k_qp_drow: the short rows of a workgroup
// through the LDS tile), and in the same kernel one thread per non-zero of the workgroup's rows in storage order (its row by bisection among
// the workgroup's row pointers in LDS, its 1..H quotients phi / d at bits_excl[i], so neighbouring lanes store to adjacent places).
// Models 1-3: the per-step chain of quant_model.inc run once with a weight of one in every row (k_qm_gh .. k_qm_row: the segments then hold the
// gene factor over the segment's divisor), and a twin of k_qm_coef that writes the factor product itself (k_qp_post): rows of weight 0 and
// entries with phi = 0 come out as defined, no division by phi.  Model 1's Phi_gh / D_h are left by k_qm_seg1 in `post` itself.
// Every sum by one thread in index order or by one workgroup with q_block_sum's tree: the result is a function of the inputs alone.
namespace {
enum : u32 { QP_ERR_THETA = 8u };
const ErrBit QP_ERRS[] = {
    {Q_ERR_SCALE, ECB_ERR_CONTRACT, "ecquant: an entry of scale is NaN, infinite or negative"},
    {QP_ERR_THETA, ECB_ERR_CONTRACT, "ecposterior: an entry of theta is NaN, infinite or negative"},
    {Q_ERR_GENE, ECB_ERR_CONTRACT, "ecquant: a gene id outside [0, n_genes)"},
};
// row e: listed when it is long
__global__ __launch_bounds__(TPB) void k_qp_rows(const int* indptr, u32 n_ecs, u32* n_long, u32* long_rows) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e < n_ecs && (u32)(indptr[e + 1] - indptr[e]) > Q_LONG_ROW) long_rows[atomicAdd(n_long, 1u)] = (u32)e;
}
__global__ __launch_bounds__(TPB) void k_qp_ones(u64* ww, u32 n_ecs) {
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    if (e < n_ecs) ww[e] = 1ull;
}
// d[e] of the short rows: k_q_estep's pass (workgroup b has rows [b TPB, (b + 1) TPB), their non-zeros go through LDS Q_TILE at a time,
// lane e adds those of its row in index order) with the sum kept.  EMIT (the flat model): the workgroup then goes over its stretch of A once
// more -- thread k has non-zeros k, k + TPB, ... in storage order, each one's row found by bisection among the workgroup's TPB + 1 row pointers
// in LDS (a row above Q_LONG_ROW among them: k_qp_dlong, launched before, has left its d) -- and writes the quotients phi / d[e], lowest bit
// first, at bits_excl[i]: neighbouring lanes store to adjacent places, and A comes from L2 the second time
template <bool EMIT>
__global__ __launch_bounds__(TPB) void k_qp_drow(const int* indptr, u32 n_ecs, const int* indices, const int* data, const double* phi, u32 n_haps,
                                                 const u32* bits_excl, double* d_out, double* post) {
    __shared__ double v[Q_TILE];
    __shared__ double dl[EMIT ? TPB : 1];
    __shared__ u32 rp[EMIT ? TPB + 1 : 1];
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
    if (mine) d_out[e] = d;
    if (!EMIT) return;
    dl[threadIdx.x] = mine ? d : e < n_ecs ? d_out[e] : 0.0;
    rp[threadIdx.x] = e < n_ecs ? a : hi;
    if (threadIdx.x == 0) rp[TPB] = hi;
    __syncthreads();
    for (u32 i = lo + threadIdx.x; i < hi; i += TPB) {
        u32 l = 0, h = TPB;                      // the first k in [0, TPB] with rp[k] > i (rp[0] = lo <= i < hi = rp[TPB]); empty rows share a pointer with the row after them
        while (l < h) { const u32 m = (l + h) >> 1; if (rp[m] <= i) l = m + 1; else h = m; }
        const double de = dl[l - 1u];
        const double* p = phi + (u64)(u32)indices[i] * n_haps;
        u32 at = bits_excl[i];
        for (u32 m = (u32)data[i]; m; m &= m - 1u, ++at) post[at] = de > 0.0 ? p[__ffs((int)m) - 1] / de : 0.0;
    }
}
// d[e] of long row long_rows[b]: k_q_elong's sum -- thread k adds non-zeros k, k + TPB, ... in that order, the tree folds the TPB sums
__global__ __launch_bounds__(TPB) void k_qp_dlong(const u32* long_rows, const int* indptr, const int* indices, const int* data, const double* phi,
                                                  u32 n_haps, double* d_out) {
    __shared__ double s[TPB];
    const u32 e = long_rows[blockIdx.x];
    const u32 a = (u32)indptr[e], b = (u32)indptr[e + 1];
    double d = 0.0;
    for (u32 i = a + threadIdx.x; i < b; i += TPB) d = q_bits_sum(phi, n_haps, (u32)indices[i], (u32)data[i], d);
    d = q_block_sum(d, s);
    if (threadIdx.x == 0) d_out[e] = d;
}
// thread i <= nnz: bit_ptr[i] = bits_excl[i], 64 bits wide
__global__ __launch_bounds__(TPB) void k_qp_bitptr(const u32* bits_excl, u64 nnz, long long* bit_ptr) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i <= nnz) bit_ptr[i] = (long long)bits_excl[i];
}
// models 1-3, thread i: non-zero i in storage order -- the posterior of its set bits from its segment's c (the gene factor over the segment's
// divisor: k_qm_row with w = 1).  model 3: c x phi; model 2: c x Phi_t / D_t x phi; model 1: c x what k_qm_seg1 left at the bit's place x phi
template <u32 MODEL>
__global__ __launch_bounds__(TPB) void k_qp_post(u64 nnz, const u32* nz_seg, const int* indices, const int* data, const u32* bits_excl, const double* phi,
                                                 const double* phi_t, const double* seg_c, u32 n_haps, double* post) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= nnz) return;
    const u32 m0 = (u32)data[i], t = (u32)indices[i];
    const double* p = phi + (u64)t * n_haps;
    double cv = seg_c[nz_seg[i]];
    if (MODEL == 2) {
        const double dt = q_bits_sum(phi, n_haps, t, m0, 0.0);
        cv = dt > 0.0 ? cv * phi_t[t] / dt : 0.0;
    }
    u32 at = bits_excl[i];
    for (u32 m = m0; m; m &= m - 1u, ++at) {
        const double v = p[__ffs((int)m) - 1];
        post[at] = MODEL == 1 ? cv * post[at] * v : cv * v;
    }
}
// what both entry points refuse before anything else
int qp_check_args(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* indptr, const void* indices, const void* data,
                  const void* theta, uint32_t n_genes, const void* gene, uint32_t model, uint64_t n_bits, const void* post) {
    if (model < 1u || model > 4u) return fail(nullptr, ECB_ERR_ARG, "ecquant: no such model (%u: 1, 2, 3 or 4)", model);
    if ((!gene && model != 4u) || (gene && n_loci && !n_genes))
        return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no gene array, or targets and no gene)");
    if (gene && (u64)n_genes * n_haps >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x genes does not fit 31 bits");
    if (!indptr || !n_loci || !n_haps || n_haps > 31) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (nnz && (!indices || !data)) return fail(nullptr, ECB_ERR_ARG, "bad argument");
    if (n_ecs >= (1u << 31) - 1u) return fail(nullptr, ECB_ERR_LIMIT, "the matrices exceed the .bin format's int32 limits");
    if (!theta || (n_bits && !post)) return fail(nullptr, ECB_ERR_ARG, "ecposterior: bad argument (no theta, or set bits and no post)");
    if (nnz >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: 2^30 non-zeros or more");
    if ((u64)n_haps * n_loci >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x loci does not fit 31 bits");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_posterior_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                    const void* d_indices_a, const void* d_data_a, const void* d_scale, const void* d_theta, uint32_t n_genes,
                                    const void* d_gene, uint32_t model, uint64_t n_bits, void* d_post, void* d_bit_ptr, void* d_row_mass) {
    RCCHK(qp_check_args(n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, d_theta, n_genes, d_gene, model, n_bits, d_post));
    Call c(device, "ecposterior: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const bool grouped = model != 4u;
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);          // as ecb_quantify_model_device: [3] the set bits, [5] the error bits of the tables and of gene
    const u64 n_tab = (u64)n_haps * n_loci, n_gtab = grouped ? (u64)n_haps * n_genes : 0;
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *bits = c.get<u32>(CV_X0, nnz), *bits_excl = c.get<u32>(CV_X1, nnz + 1), *sums = c.get<u32>(CV_SUMS2, scan_words(nnz + 1));
    double *theta = c.get<double>(n_tab), *phi = c.get<double>(n_tab), *scale = d_scale ? c.get<double>(n_tab) : nullptr;
    u64 *gk0 = nullptr, *gk1 = nullptr;
    u32 *gv0 = nullptr, *gv1 = nullptr;
    if (grouped) { gk0 = c.get<u64>(n_loci); gk1 = c.get<u64>(n_loci); gv0 = c.get<u32>(n_loci); gv1 = c.get<u32>(n_loci); }
    if (const int rc = c.missing()) return rc;
    const int* ip = (const int*)d_indptr_a; const int* ix = (const int*)d_indices_a; const int* da = (const int*)d_data_a;
    const int* gene = (const int*)d_gene;
    CALLCHK(c, hipMemsetAsync(words, 0, n_words * 8, st));
    k_gm_check<true><<<nblk(std::max<u64>((u64)n_ecs + 1, (nnz + GM_ITEMS - 1) / GM_ITEMS), TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, nullptr, n_loci,
                                                                                                             n_haps, bits, words);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, bits, nnz, bits_excl, sums, words + 3, 1, bits_excl + nnz));
    // (into the call's own tables, T x H: nothing of the caller's is written yet)
    if (d_scale) k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_scale, n_loci, n_haps, scale, Q_ERR_SCALE, reinterpret_cast<u32*>(words + 5));
    k_q_tab<<<nblk(n_tab, TPB), TPB, 0, st>>>((const double*)d_theta, n_loci, n_haps, theta, QP_ERR_THETA, reinterpret_cast<u32*>(words + 5));
    if (gene) k_qm_gkeys<<<nblk(n_loci, TPB), TPB, 0, st>>>(gene, n_loci, n_genes, gk0, gv0, reinterpret_cast<u32*>(words + 5));
    CALLCHK(c, hipGetLastError());
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    if (back[3] >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    RCCHK(refuse_bits(nullptr, QP_ERRS, (u32)back[5]));
    if (back[3] != n_bits)
        return fail(nullptr, ECB_ERR_ARG, "ecposterior: n_bits is %llu, the matrix has %llu set bits", (unsigned long long)n_bits, (unsigned long long)back[3]);
    // the input is well formed: from here on the outputs are written
    if (d_bit_ptr) k_qp_bitptr<<<nblk(nnz + 1, TPB), TPB, 0, st>>>(bits_excl, nnz, (long long*)d_bit_ptr);
    CALLCHK(c, hipGetLastError());
    if (n_ecs && nnz) {
        double* post = (double*)d_post;
        const bool flat_d = !grouped || d_row_mass;
        const u32 n_eblk = nblk(n_ecs, TPB);
        u32 *long_rows = c.get<u32>(nnz / Q_LONG_ROW + 1), *n_long_d = c.get<u32>(2);
        double* d = !grouped && !d_row_mass ? c.get<double>(CV_X2, n_ecs) : (double*)d_row_mass;          // (from the pool: no allocation of its own when the caller takes no row_mass)
        if (const int rc = c.missing()) return rc;
        CALLCHK(c, hipMemsetAsync(n_long_d, 0, 8, st));
        k_q_phi<<<nblk(n_tab, TPB), TPB, 0, st>>>(theta, scale, n_tab, phi);
        k_qp_rows<<<n_eblk, TPB, 0, st>>>(ip, n_ecs, n_long_d, long_rows);
        CALLCHK(c, hipGetLastError());
        u32 nlr = 0;
        if (!grouped) {
            CALLCHK(c, hipMemcpyAsync(&nlr, n_long_d, 4, hipMemcpyDeviceToHost, st));
            CALLCHK(c, hipStreamSynchronize(st));
        }
        u64* n_segs_d = nullptr;
        u32 *flag = nullptr, *segid = nullptr, *seg_start = nullptr, *nz_seg = nullptr, *long_genes = nullptr;
        int *gptr = nullptr, *gmem = nullptr;
        const u64* rkeys = nullptr; const u32* gnz = nullptr;
        u32 n_segs = 0, nlg = 0;
        if (grouped) {
            // the members of each gene and the gene-ordered view of the rows with its segments, as ecb_quantify_model_device builds them
            u64 *k0 = c.get<u64>(CV_KEYS0, nnz), *k1 = c.get<u64>(CV_KEYS1, nnz);
            u32 *v0 = c.get<u32>(CV_VALS0, nnz), *v1 = c.get<u32>(CV_VALS1, nnz);
            SortScratch ss{c.get<u32>(CV_HIST, rs_words(std::max<u64>(nnz, n_loci))), c.get<u32>(CV_OFFS, RS_AUX_WORDS), words + 4};
            long_genes = c.get<u32>(n_loci / Q_LONG_GENE + 1);
            gptr = c.get<int>((u64)n_genes + 1); gmem = c.get<int>(n_loci);
            flag = c.get<u32>(nnz); segid = c.get<u32>(nnz + 1); seg_start = c.get<u32>(nnz + 1); nz_seg = c.get<u32>(nnz);
            n_segs_d = c.get<u64>(1);
            if (const int rc = c.missing()) return rc;
            SortBufs sg{{gk0, gk1}, {gv0, gv1}};
            CALLCHK(c, radix_sort_pairs64(st, sg, n_loci, ss, msb_mask(n_genes - 1) << 32));
            k_split_out<<<nblk(n_loci, TPB), TPB, 0, st>>>(sg.keys(), sg.vals(), n_loci, gmem, gmem);
            k_row_ptr<<<nblk((u64)n_genes + 1, TPB), TPB, 0, st>>>(sg.keys(), n_loci, n_genes, gptr);
            k_qm_glist<<<nblk(n_genes, TPB), TPB, 0, st>>>(gptr, n_genes, n_long_d + 1, long_genes);
            k_qm_rkeys<<<n_eblk, TPB, 0, st>>>(ip, n_ecs, ix, gene, k0, v0);
            SortBufs s{{k0, k1}, {v0, v1}};
            CALLCHK(c, radix_sort_pairs64(st, s, nnz, ss, msb_mask(n_ecs - 1) << 32 | msb_mask(n_genes - 1)));
            rkeys = s.keys(); gnz = s.vals();
            k_run_heads<<<nblk(nnz, TPB), TPB, 0, st>>>(rkeys, nnz, flag);
            CALLCHK(c, scan_launch(st, flag, nnz, segid, sums, n_segs_d, 1, segid + nnz));
            k_qm_segs<<<nblk(nnz + 1, TPB), TPB, 0, st>>>(flag, segid, gnz, nnz, seg_start, nz_seg);
            CALLCHK(c, hipGetLastError());
            u32 cnt[2] = {0, 0};
            u64 n_segs64 = 0;
            CALLCHK(c, hipMemcpyAsync(cnt, n_long_d, 8, hipMemcpyDeviceToHost, st));
            CALLCHK(c, hipMemcpyAsync(&n_segs64, n_segs_d, 8, hipMemcpyDeviceToHost, st));
            CALLCHK(c, hipStreamSynchronize(st));
            nlr = cnt[0]; nlg = cnt[1]; n_segs = (u32)n_segs64;
        }
        if (flat_d) {
            if (nlr) k_qp_dlong<<<nlr, TPB, 0, st>>>(long_rows, ip, ix, da, phi, n_haps, d);
            if (grouped) k_qp_drow<false><<<n_eblk, TPB, 0, st>>>(ip, n_ecs, ix, da, phi, n_haps, bits_excl, d, nullptr);
            else k_qp_drow<true><<<n_eblk, TPB, 0, st>>>(ip, n_ecs, ix, da, phi, n_haps, bits_excl, d, post);
        }
        if (grouped) {
            u64* ww = c.get<u64>(n_ecs);
            double *phi_gh = c.get<double>(n_gtab), *phi_g = c.get<double>(n_genes), *phi_t = model == 2u ? c.get<double>(n_loci) : nullptr;
            double *seg_c = c.get<double>(nnz), *seg_x = c.get<double>(nnz);
            u64* expl_parts = c.get<u64>((u64)n_eblk + nnz / Q_LONG_ROW + 1);
            QState* qs = c.get<QState>(1);
            if (const int rc = c.missing()) return rc;
            u32 hp = 1;
            while (hp < n_haps) hp <<= 1;
            CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QState), st));          // (done = 0: the chain's kernels run)
            k_qp_ones<<<n_eblk, TPB, 0, st>>>(ww, n_ecs);
            k_qm_gh<<<nblk(n_gtab, TPB), TPB, 0, st>>>(qs, gptr, gmem, phi, n_genes, n_haps, phi_gh);
            if (nlg) k_qm_ghlong<<<nlg, TPB, 0, st>>>(qs, long_genes, gptr, gmem, phi, n_haps, hp, phi_gh);
            k_qm_g<<<nblk((u64)n_genes + (phi_t ? n_loci : 0u), TPB), TPB, 0, st>>>(qs, phi_gh, phi, n_genes, n_loci, n_haps, phi_g, phi_t);
            if (model == 1u)
                k_qm_seg1<<<nblk((u64)n_segs * hp, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, bits_excl, phi, phi_gh, phi_g, n_haps, hp,
                                                                      seg_c, seg_x, post);
            else if (model == 2u)
                k_qm_seg<2><<<nblk(n_segs, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, phi, phi_g, phi_t, n_haps, seg_c, seg_x);
            else k_qm_seg<3><<<nblk(n_segs, TPB), TPB, 0, st>>>(qs, seg_start, n_segs, rkeys, gnz, ix, da, phi, phi_g, phi_t, n_haps, seg_c, seg_x);
            if (nlr) k_qm_rowlong<<<nlr, TPB, 0, st>>>(qs, long_rows, ip, segid, seg_x, ww, seg_c, expl_parts + n_eblk);
            k_qm_row<<<n_eblk, TPB, 0, st>>>(qs, ip, n_ecs, segid, seg_x, ww, seg_c, expl_parts);
            if (model == 1u) k_qp_post<1><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, post);
            else if (model == 2u) k_qp_post<2><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, post);
            else k_qp_post<3><<<nblk(nnz, TPB), TPB, 0, st>>>(nnz, nz_seg, ix, da, bits_excl, phi, phi_t, seg_c, n_haps, post);
        }
        CALLCHK(c, hipGetLastError());
    }
    CALLCHK(c, hipStreamSynchronize(st));
    return ECB_OK;
}

extern "C" int ecb_posterior(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                             const int32_t* indices_a, const int32_t* data_a, const double* scale, const double* theta, uint32_t n_genes,
                             const int32_t* gene, uint32_t model, uint64_t n_bits, double* post, int64_t* bit_ptr, double* row_mass) {
    RCCHK(qp_check_args(n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, theta, n_genes, gene, model, n_bits, post));
    Call c(device, "ecposterior: "); if (c.rc) return c.rc;
    const u64 plane = (u64)n_haps * n_loci * 8;
    // room for post: the set bits the masks hold, counted here (one pass over nnz words), not what the caller says there are -- a wrong n_bits
    // is the device entry point's refusal, with both numbers, after everything it refuses on A
    u64 have = 0;
    for (u64 i = 0; i < nnz; ++i) have += (u64)__builtin_popcount((unsigned)data_a[i]);
    if (have >= (1ull << 32)) return fail(nullptr, ECB_ERR_LIMIT, "more than 2^32-1 set haplotype bits");
    DevBuf<> ipa, ixa, daa, sc, th, gn, po, bp, rm;
    std::vector<StageIn> in = {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz * 4}, {&daa, data_a, nnz * 4}, {&th, theta, plane},
                               {&po, nullptr, have * 8}};
    if (scale) in.push_back({&sc, scale, plane});
    if (gene) in.push_back({&gn, gene, (u64)n_loci * 4});
    if (bit_ptr) in.push_back({&bp, nullptr, (nnz + 1) * 8});
    if (row_mass) in.push_back({&rm, nullptr, (u64)n_ecs * 8});
    int rc = stage_in(c, in);
    if (rc == ECB_OK) rc = ecb_posterior_device(device, n_ecs, n_loci, n_haps, nnz, ipa.p, ixa.p, daa.p, sc.p, th.p, n_genes, gn.p, model, n_bits, po.p,
                                                bp.p, rm.p);
    RCCHK(rc);
    const bool any = n_ecs && nnz;
    return stage_out(c, {{bit_ptr, &bp, bit_ptr ? (nnz + 1) * 8 : 0}, {post, &po, any ? n_bits * 8 : 0}, {row_mass, &rm, any && row_mass ? (u64)n_ecs * 8 : 0}});
}
