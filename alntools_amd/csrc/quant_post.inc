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
// Host side: quant.inc's q_front without N (theta refused in this entry point's words, the n_bits mismatch after everything else), and for
// models 1-3 quant_model.inc's qm_gene_view, qm_tables and qm_step with `post` set; the row kernels run quant.inc's q_tile_pass and q_long_row_sum.
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
    const double d = q_tile_pass<Q_TILE>(v, phi, n_haps, indices, data, lo, hi, a, b, mine);
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
    const double d = q_long_row_sum(s, phi, n_haps, indices, data, (u32)indptr[e], (u32)indptr[e + 1]);
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
    const QMat m{n_ecs, n_loci, n_haps, nnz, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a, 0, 0, nullptr, nullptr, nullptr};
    const QModel mdl{model, n_genes, (const int*)d_gene};
    const u64 n_tab = (u64)n_haps * n_loci;
    // the front without N: no weights; theta is the caller's, refused in this entry point's words; the genes checked whenever they are given
    QFront f;
    RCCHK(q_front(c, m, -1, d_scale, d_theta, QP_ERR_THETA, true, mdl.gene, n_genes, grouped, nnz + 1, QP_ERRS, f));
    if (f.n_bits != n_bits)
        return fail(nullptr, ECB_ERR_ARG, "ecposterior: n_bits is %llu, the matrix has %llu set bits", (unsigned long long)n_bits, (unsigned long long)f.n_bits);
    // the input is well formed: from here on the outputs are written
    if (d_bit_ptr) k_qp_bitptr<<<nblk(nnz + 1, TPB), TPB, 0, st>>>(f.bits_excl, nnz, (long long*)d_bit_ptr);
    CALLCHK(c, hipGetLastError());
    if (n_ecs && nnz) {
        double* post = (double*)d_post;
        const u32 n_eblk = nblk(n_ecs, TPB);
        u32 *long_rows = c.get<u32>(nnz / Q_LONG_ROW + 1), *n_long_d = c.get<u32>(1);
        double* d = !grouped && !d_row_mass ? c.get<double>(CV_X2, n_ecs) : (double*)d_row_mass;          // (from the pool: no allocation of its own when the caller takes no row_mass)
        if (const int rc = c.missing()) return rc;
        CALLCHK(c, hipMemsetAsync(n_long_d, 0, 4, st));
        k_q_phi<<<nblk(n_tab, TPB), TPB, 0, st>>>(f.theta, f.scale, n_tab, f.phi);
        k_qp_rows<<<n_eblk, TPB, 0, st>>>(m.ip, n_ecs, n_long_d, long_rows);
        CALLCHK(c, hipGetLastError());
        // models 1-3: the members of each gene and the gene-ordered view of the rows with its segments, as ecb_quantify_model_device has them
        QmTabs mt{};
        if (grouped) {
            QSort srt = q_sort_bufs(c, nnz, std::max<u64>(nnz, n_loci), f.words + 4);
            if (const int rc = c.missing()) return rc;
            RCCHK(qm_gene_view(c, m, f, mdl.gene, n_genes, srt, mt.g));
        }
        u32 nlr = 0;
        u64 gcnt[2] = {0, 0};
        CALLCHK(c, hipMemcpyAsync(&nlr, n_long_d, 4, hipMemcpyDeviceToHost, st));
        if (grouped) CALLCHK(c, hipMemcpyAsync(gcnt, mt.g.cnt, 16, hipMemcpyDeviceToHost, st));
        CALLCHK(c, hipStreamSynchronize(st));
        mt.g.n_segs = (u32)gcnt[0]; mt.g.n_long_genes = (u32)gcnt[1];
        if (!grouped || d_row_mass) {
            if (nlr) k_qp_dlong<<<nlr, TPB, 0, st>>>(long_rows, m.ip, m.ix, m.da, f.phi, n_haps, d);
            if (grouped) k_qp_drow<false><<<n_eblk, TPB, 0, st>>>(m.ip, n_ecs, m.ix, m.da, f.phi, n_haps, f.bits_excl, d, nullptr);
            else k_qp_drow<true><<<n_eblk, TPB, 0, st>>>(m.ip, n_ecs, m.ix, m.da, f.phi, n_haps, f.bits_excl, d, post);
        }
        if (grouped) {
            // the chain once, with a weight of one in every row and a state that says "running"
            // (its tables allocated here, while the row kernels run; model 1's Phi_gh / D_h are left in `post` itself)
            u64 *ww = c.get<u64>(n_ecs), *expl_parts = c.get<u64>((u64)n_eblk + nnz / Q_LONG_ROW + 1);
            QState* qs = c.get<QState>(1);
            RCCHK(qm_tables(c, m, f, mdl, post, mt));
            QView v{};
            v.st = st; v.n_ecs = n_ecs; v.n_loci = n_loci; v.n_haps = n_haps; v.n_eblk = n_eblk; v.nlr = nlr; v.nnz = nnz;
            v.ip = m.ip; v.ix = m.ix; v.da = m.da; v.bits_excl = f.bits_excl; v.long_rows = long_rows; v.ww = ww; v.qs = qs; v.phi = f.phi;
            v.expl_parts = expl_parts;
            for (v.hp = 1; v.hp < n_haps;) v.hp <<= 1;
            CALLCHK(c, hipMemsetAsync(qs, 0, sizeof(QState), st));          // (done = 0: the chain's kernels run)
            k_qp_ones<<<n_eblk, TPB, 0, st>>>(ww, n_ecs);
            qm_step(v, mt, model, true);
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
    QStage b;
    DevBuf<> sc, th, gn, po, bp, rm;
    std::vector<StageIn> in = q_stage(b, QMat{n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, 0, 0, nullptr, nullptr, nullptr});
    in.insert(in.end(), {{&th, theta, plane}, {&po, nullptr, have * 8}});
    if (scale) in.push_back({&sc, scale, plane});
    if (gene) in.push_back({&gn, gene, (u64)n_loci * 4});
    if (bit_ptr) in.push_back({&bp, nullptr, (nnz + 1) * 8});
    if (row_mass) in.push_back({&rm, nullptr, (u64)n_ecs * 8});
    RCCHK(stage_in(c, in));
    RCCHK(ecb_posterior_device(device, n_ecs, n_loci, n_haps, nnz, b.ipa.p, b.ixa.p, b.daa.p, sc.p, th.p, n_genes, gn.p, model, n_bits, po.p, bp.p, rm.p));
    const bool any = n_ecs && nnz;
    return stage_out(c, {{bit_ptr, &bp, bit_ptr ? (nnz + 1) * 8 : 0}, {post, &po, any ? n_bits * 8 : 0}, {row_mass, &rm, any && row_mass ? (u64)n_ecs * 8 : 0}});
}
