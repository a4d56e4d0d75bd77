// ---- ecboot: bootstrap replicates of N, drawn on the device, and the moments of their estimates (ecb_resample* / ecb_quantify_bootstrap*;
// included by ecb.hip after quant_post.inc, boot_draw.h before it) ---------------------------------------------------------------------------
// Replicate b redraws the W = sum of w[e] reads of N's column `sample` (-1: pooled) with replacement: draw i is Philox4x32-10 at counter
// (i >> 1, 0, b, 0) under the key (seed) -- both 64-bit halves of a call are used -- scaled to x = (u W) >> 64, and lands on the row e with
// cum[e - 1] <= x < cum[e].  Everything is an integer: the counts of a replicate are a function of (N, sample, seed, b) alone.
// Set-up, once per call: k_ca_weights (count-alignments' weights and its check of N), k_bs_w32 (the weights as 32-bit words, W by one integer
// add per workgroup), the library's scan (excl: E + 1 exclusive prefix sums, cum[e] = excl[e + 1]), k_bs_guide (guide[g] = the row of
// x = g << shift for the G + 1 bucket edges, G = the power of two at or above E: a draw bisects excl between guide[x >> shift] and
// guide[(x >> shift) + 1] only, so its walk is bounded whatever the weights).
// Per batch of replicates (replicates x E below 2^31 and inside the budget): k_bs_draw, grid (chunks of BS_WG_DRAWS draws, replicates): a
// thread takes BS_DRAWS consecutive draws of one replicate -- BS_DRAWS / 2 whole Philox calls -- and adds 1 to table[replicate][row] with an
// integer atomic (exact in any order).  Lanes of a wave that hit the row of the wave's first waiting lane become one add of their number
// (BS_AGG_ROUNDS rounds of it; what is left adds on its own): a heavy EC is one address, and 64 adds to it would queue up.
// Then k_bs_flag, the library's scan, k_bs_emit: the table compacted into a CSC N of one column per replicate, rows ascending, no zeros.
// The bootstrap is a composition, no EM of its own: per batch, the replicates as a multisample N through qc_run (the support, then
// ecquant-cells' EM, flat or with a model), then k_bs_moments -- thread t: for every replicate of the batch in order, locus t found by
// bisection among the replicate's slots, Welford's update of (m, M) for every h and, over y = the sum of x over h ascending, of the totals.
// The (m, M) tables carry across batches, so the result does not depend on how the replicates are batched.
namespace {
constexpr u32 BS_DRAWS = 8;                          // consecutive draws of one replicate per thread of k_bs_draw (even: whole Philox calls)
constexpr u32 BS_WG_DRAWS = TPB * BS_DRAWS;          // draws per workgroup of k_bs_draw
constexpr u32 BS_AGG_ROUNDS = 2;                     // rounds of wave aggregation before the lanes left add on their own
constexpr u32 BS_MAX_REPS = 32768;                   // replicates per batch at most (k_bs_draw's grid.y)
constexpr u64 BS_CELL_BYTES = 12;                    // device bytes a batch holds per (replicate, EC): table, flag, pos
static_assert(BS_DRAWS % 2u == 0u, "whole Philox calls");

// row e: its weight as a 32-bit word (capped: a W that large is refused before anything reads it), the workgroup's sum added to *w_total
__global__ __launch_bounds__(TPB) void k_bs_w32(const u64* ww, u32 n_ecs, u32* w32, u64* w_total) {
    __shared__ u64 s[TPB];
    const u64 e = blockIdx.x * (u64)TPB + threadIdx.x;
    u64 w = 0;
    if (e < n_ecs) { w = ww[e] & CA_WEIGHT; w32[e] = (u32)std::min<u64>(w, 0xFFFFFFFFull); }
    w = q_block_sum(w, s);
    if (threadIdx.x == 0 && w) atomicAdd(reinterpret_cast<unsigned long long*>(w_total), (unsigned long long)w);
}
// bucket edge g <= G: the row x = g << shift lands on (the last e with excl[e] <= x: rows of weight 0 share a prefix with the row after
// them and are passed over); an edge at or beyond W: the last row
__global__ __launch_bounds__(TPB) void k_bs_guide(const u32* excl, u32 n_ecs, u32 W, u32 shift, u32 G, u32* guide) {
    const u64 g = blockIdx.x * (u64)TPB + threadIdx.x;
    if (g > G) return;
    const u64 x = g << shift;
    guide[g] = x >= W ? n_ecs - 1u : qc_last_le(excl, 0u, n_ecs - 1u, x);
}
// one draw of every lane of the wave (valid: this lane has one) added to col[row]: the lanes that share the first waiting lane's row
// become one add
__device__ __forceinline__ void bs_add(u32* col, u32 row, bool valid) {
    const u32 lane = threadIdx.x & 63u;
    u64 left = __ballot(valid);
    for (u32 r = 0; r < BS_AGG_ROUNDS && left; ++r) {
        const int lead = __ffsll((long long)left) - 1;
        const u32 lr = (u32)__shfl((int)row, lead);
        const u64 same = __ballot(valid && row == lr) & left;
        if ((int)lane == lead) atomicAdd(col + lr, (u32)__popcll(same));
        left &= ~same;
    }
    if ((left >> lane) & 1ull) atomicAdd(col + row, 1u);
}
// workgroup (chunk, r): draws [chunk BS_WG_DRAWS, (chunk + 1) BS_WG_DRAWS) of replicate b0 + r, thread k its BS_DRAWS consecutive ones
__global__ __launch_bounds__(TPB) void k_bs_draw(const u32* excl, const u32* guide, u32 n_ecs, u32 W, u32 shift, u64 seed, u32 b0, u32* table) {
    const u32 b = b0 + blockIdx.y;
    u32* col = table + (u64)blockIdx.y * n_ecs;
    const u64 i0 = ((u64)blockIdx.x * TPB + threadIdx.x) * BS_DRAWS;
#pragma unroll
    for (u32 p = 0; p < BS_DRAWS / 2u; ++p) {
        const u64 i = i0 + 2u * p;
        BsPhilox o{};
        if (i < W) o = bs_pair(seed, b, (u32)(i >> 1));
#pragma unroll
        for (u32 half = 0; half < 2u; ++half) {
            const bool valid = i + half < W;
            u32 row = 0;
            if (valid) {
                const u32 x = bs_x(o, half, W), g = x >> shift;
                row = qc_last_le(excl, guide[g], guide[g + 1u], x);
            }
            bs_add(col, row, valid);
        }
    }
}
__global__ __launch_bounds__(TPB) void k_bs_flag(const u32* table, u64 n, u32* flag) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k < n) flag[k] = table[k] != 0u;
}
// cell k = replicate r x E + row: its count, when it has one, at pos[k] (+ base: the entries of the batches before); the replicate's
// column pointer by the thread of its first row, the last one by thread 0
__global__ __launch_bounds__(TPB) void k_bs_emit(const u32* table, const u32* pos, u64 n, u32 n_ecs, u32 n_reps, const u64* d_total, u32 base,
                                                 int* rep_ptr, int* rep_ec, int* rep_count) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k == 0) rep_ptr[n_reps] = (int)(base + (u32)*d_total);
    if (k >= n) return;
    const u32 r = (u32)(k / n_ecs), e = (u32)(k - (u64)r * n_ecs), v = table[k];
    if (e == 0) rep_ptr[r] = (int)(base + pos[k]);
    if (v && rep_ec) { rep_ec[pos[k]] = (int)e; rep_count[pos[k]] = (int)v; }
}
__global__ __launch_bounds__(TPB) void k_bs_fill_ptr(int* rep_ptr, u64 n, int v) {
    const u64 k = blockIdx.x * (u64)TPB + threadIdx.x;
    if (k < n) rep_ptr[k] = v;
}
// thread t: locus t through the batch's replicates in order (replicate r is number done + r of the call): x[h] = theta at the slot of t in
// the replicate's support, 0 when it has none; Welford's update of (m, M)[h, t]; y = the sum of x[h], h ascending, and the same update of the
// totals; x to reps when the caller keeps them
__global__ __launch_bounds__(TPB) void k_bs_moments(const long long* cell_ptr, const int* slot_locus, const double* theta, u32 n_batch, u32 done,
                                                    u32 n_loci, u32 n_haps, double* m, double* M, double* tm, double* tM, double* reps) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t >= n_loci) return;
    const u64 plane = (u64)n_haps * n_loci;
    for (u32 r = 0; r < n_batch; ++r) {
        const u64 a = (u64)cell_ptr[r], z = (u64)cell_ptr[r + 1];
        u64 lo = a, hi = z;                            // the first slot of [a, z) whose locus is at or above t
        while (lo < hi) { const u64 mid = (lo + hi) / 2u; if ((u32)slot_locus[mid] < (u32)t) lo = mid + 1u; else hi = mid; }
        const bool have = lo < z && (u32)slot_locus[lo] == (u32)t;
        const double cnt = (double)(done + r + 1u);
        double y = 0.0;
        for (u32 h = 0; h < n_haps; ++h) {
            const double x = have ? theta[lo * n_haps + h] : 0.0;
            const u64 at = (u64)h * n_loci + t;
            const double d = x - m[at], mn = m[at] + d / cnt;
            m[at] = mn;
            M[at] += d * (x - mn);
            y += x;
            if (reps) reps[(u64)r * plane + at] = x;
        }
        const double d = y - tm[t], mn = tm[t] + d / cnt;
        tm[t] = mn;
        tM[t] += d * (y - mn);
    }
}
// mean = m, sd = sqrt(M / (B - 1)), 0 when B = 1
__global__ __launch_bounds__(TPB) void k_bs_finish(const double* m, const double* M, u64 n, u32 n_reps, double* mean, double* sd) {
    const u64 i = blockIdx.x * (u64)TPB + threadIdx.x;
    if (i >= n) return;
    mean[i] = m[i];
    sd[i] = n_reps > 1u ? sqrt(M[i] / (double)(n_reps - 1u)) : 0.0;
}

// N as both entry points of ecb_resample take it: what they refuse before anything is allocated
int bs_check_n(uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int64_t sample) {
    if (!indptr_n || !n_samples || (nnz_n && (!indices_n || !data_n))) return fail(nullptr, ECB_ERR_ARG, "ecboot: bad argument (no N, or no sample)");
    if (n_ecs >= (1u << 31) - 1u || nnz_n >= (1ull << 31) || n_samples >= (1u << 31) - 1u)
        return fail(nullptr, ECB_ERR_LIMIT, "the matrices exceed the .bin format's int32 limits");
    if (sample < -1 || sample >= (int64_t)n_samples) return fail(nullptr, ECB_ERR_CONTRACT, "ecboot: no such sample (%lld of %u)", (long long)sample, n_samples);
    return ECB_OK;
}
int bs_check_resample(uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int64_t sample,
                      uint64_t b0, uint32_t n_reps, const void* rep_ptr) {
    RCCHK(bs_check_n(n_ecs, n_samples, nnz_n, indptr_n, indices_n, data_n, sample));
    if (!rep_ptr) return fail(nullptr, ECB_ERR_ARG, "ecboot: bad argument (no rep_ptr)");
    if (b0 + n_reps > (1ull << 32) || b0 >= (1ull << 32)) return fail(nullptr, ECB_ERR_ARG, "ecboot: replicate numbers beyond 2^32 - 1 (b0 + n_reps)");
    if (n_reps >= (1u << 31) - 1u) return fail(nullptr, ECB_ERR_LIMIT, "ecboot: 2^31 - 1 replicates or more");
    return ECB_OK;
}

// what a call draws from: the prefix sums of the weights and the guide over x (all in the call's own buffers: a bootstrap runs other
// calls, which take the pool, while it holds these)
struct BsPlan { u32 n_ecs, W, shift, G; u32 *excl, *guide; u64* words; };
int bs_front(Call& c, u32 n_ecs, u32 n_samples, u64 nnz_n, const int* pn, const int* xn, const int* dn, int64_t sample, BsPlan& p) {
    hipStream_t st = c.st;
    p = BsPlan{n_ecs, 0, 0, 1, nullptr, nullptr, nullptr};
    while (p.G < n_ecs) p.G <<= 1;
    p.words = c.get<u64>(8);                           // [1] the error bits of N, [2] W, [3] a scan's total
    u64* ww = c.get<u64>(n_ecs);
    u32* w32 = c.get<u32>(n_ecs);
    p.excl = c.get<u32>((u64)n_ecs + 1);
    p.guide = c.get<u32>((u64)p.G + 1);
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, hipMemsetAsync(p.words, 0, 64, st));
    CALLCHK(c, hipMemsetAsync(ww, 0, std::max<u64>(n_ecs, 1) * 8, st));
    k_ca_weights<<<nblk(std::max<u64>(nnz_n, (u64)n_samples + 1), TPB), TPB, 0, st>>>(pn, n_samples, xn, dn, nnz_n, n_ecs, sample, ww, p.words);
    if (n_ecs) k_bs_w32<<<nblk(n_ecs, TPB), TPB, 0, st>>>(ww, n_ecs, w32, p.words + 2);
    CALLCHK(c, hipGetLastError());
    u64 back[8];
    if (const int rc = c.read_back(back, p.words, 8)) return rc;
    RCCHK(refuse_bits(nullptr, CA_ERRS, (u32)back[1]));
    if (back[2] >= (1ull << 31))
        return fail(nullptr, ECB_ERR_LIMIT, "ecboot: W is %llu: a replicate's count must fit N's int32 (2^31 reads or more)", (unsigned long long)back[2]);
    p.W = (u32)back[2];
    if (!p.W) return ECB_OK;
    while (((u64)(p.W - 1u) >> p.shift) >= p.G) ++p.shift;
    u32* sums = c.get<u32>(scan_words(n_ecs));
    if (const int rc = c.missing()) return rc;
    CALLCHK(c, scan_launch(st, w32, n_ecs, p.excl, sums, nullptr, 1, p.excl + n_ecs));
    k_bs_guide<<<nblk((u64)p.G + 1, TPB), TPB, 0, st>>>(p.excl, n_ecs, p.W, p.shift, p.G, p.guide);
    CALLCHK(c, hipGetLastError());
    return ECB_OK;
}
// replicates per batch: replicates x E below 2^31, inside the budget (0: half of what is free), one at the least
int bs_batch_reps(Call& c, const BsPlan& p, u64 budget_bytes, u32 n_reps, u32& per) {
    if (!budget_bytes) {
        size_t fr = 0, tot = 0;
        CALLCHK(c, hipMemGetInfo(&fr, &tot));
        budget_bytes = std::max<u64>(fr / 2, 1);
    }
    const u64 E = std::max<u32>(p.n_ecs, 1u), cells = std::min<u64>((1ull << 31) - 1, budget_bytes / BS_CELL_BYTES);
    per = (u32)std::max<u64>(1, std::min<u64>(std::min<u64>(n_reps, BS_MAX_REPS), cells / E));
    return ECB_OK;
}
// a batch's scratch, sized once for the largest batch
struct BsBufs { u32 *table, *flag, *pos, *sums; };
int bs_bufs(Call& c, const BsPlan& p, u32 per, BsBufs& b) {
    const u64 n = (u64)per * p.n_ecs;
    b = BsBufs{c.get<u32>(n), c.get<u32>(n), c.get<u32>(n), c.get<u32>(scan_words(n))};
    return c.missing();
}
// replicates [b, b + R) drawn and counted: table, and pos = where each cell's entry goes; *nnz = the batch's entries (one wait)
int bs_draw_batch(Call& c, const BsPlan& p, const BsBufs& b, u64 seed, u32 first, u32 R, u64& nnz) {
    hipStream_t st = c.st;
    const u64 n = (u64)R * p.n_ecs;
    CALLCHK(c, hipMemsetAsync(b.table, 0, std::max<u64>(n, 1) * 4, st));
    k_bs_draw<<<dim3(nblk(p.W, BS_WG_DRAWS), R), TPB, 0, st>>>(p.excl, p.guide, p.n_ecs, p.W, p.shift, seed, first, b.table);
    k_bs_flag<<<nblk(n, TPB), TPB, 0, st>>>(b.table, n, b.flag);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, b.flag, n, b.pos, b.sums, p.words + 3));
    return c.read_back(&nnz, p.words + 3, 1);
}
void bs_emit(Call& c, const BsPlan& p, const BsBufs& b, u32 R, u32 base, int* rep_ptr, int* rep_ec, int* rep_count) {
    const u64 n = (u64)R * p.n_ecs;
    k_bs_emit<<<nblk(n, TPB), TPB, 0, c.st>>>(b.table, b.pos, n, p.n_ecs, R, p.words + 3, base, rep_ptr, rep_ec, rep_count);
}

// the arguments of the bootstrap, checked before anything is allocated: ecb_quantify_model's refusals, then its own
int bs_check_boot(const QMat& m, int64_t sample, double tol, uint32_t n_genes, const void* gene, uint32_t model, uint32_t n_reps, const void* mean,
                  const void* sd) {
    if (model < 1u || model > 4u) return fail(nullptr, ECB_ERR_ARG, "ecquant: no such model (%u: 1, 2, 3 or 4)", model);
    if ((!gene && model != 4u) || (gene && m.n_loci && !n_genes))
        return fail(nullptr, ECB_ERR_ARG, "ecquant: bad argument (no gene array, or targets and no gene)");
    if (gene && (u64)n_genes * m.n_haps >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x genes does not fit 31 bits");
    RCCHK(ca_check_matrices(m.n_ecs, m.n_loci, m.n_haps, m.nnz, m.ip, m.ix, m.da, m.n_samples, m.nnz_n, m.pn, m.xn, m.dn));
    if (!mean || !sd || !(tol >= 0.0) || !n_reps)
        return fail(nullptr, ECB_ERR_ARG, "ecboot: bad argument (no mean or sd, no replicate, or a tolerance that is NaN or negative)");
    if (m.nnz >= (1ull << 30)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: 2^30 non-zeros or more");
    if ((u64)m.n_haps * m.n_loci >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecquant: haplotypes x loci does not fit 31 bits");
    if (sample < -1 || sample >= (int64_t)m.n_samples)
        return fail(nullptr, ECB_ERR_CONTRACT, "ecquant: no such sample (%lld of %u)", (long long)sample, m.n_samples);
    if (n_reps >= (1u << 31) - 1u) return fail(nullptr, ECB_ERR_LIMIT, "ecboot: 2^31 - 1 replicates or more");
    return ECB_OK;
}
struct BsOut { void *mean, *sd, *tot_mean, *tot_sd, *reps, *n_iter, *delta, *explained, *converged; };      // device memory; from tot_mean on may be null
// Both entry points of the bootstrap, their arguments checked, every array on the device
int bs_boot_run(int device, const QMat& m, int64_t sample, const void* d_scale, u32 max_iters, double tol, u64 budget_bytes, const QModel& mdl, u64 seed,
                u32 n_reps, const BsOut& o) {
    Call c(device, "ecboot: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u32 n_loci = m.n_loci, n_haps = m.n_haps;
    const u64 plane = (u64)n_haps * n_loci;
    BsPlan p;
    RCCHK(bs_front(c, m.n_ecs, m.n_samples, m.nnz_n, m.pn, m.xn, m.dn, sample, p));
    u32 per = 1;
    RCCHK(bs_batch_reps(c, p, budget_bytes, n_reps, per));
    BsBufs b;
    RCCHK(bs_bufs(c, p, p.W ? per : 0u, b));
    double *mm = c.get<double>(plane), *MM = c.get<double>(plane), *tm = c.get<double>(n_loci), *tM = c.get<double>(n_loci);
    int* rep_ptr = c.get<int>((u64)per + 1);
    long long* cell_ptr = c.get<long long>((u64)per + 1);
    if (const int rc = c.missing()) return rc;
    for (double* t : {mm, MM}) CALLCHK(c, hipMemsetAsync(t, 0, plane * 8, st));
    for (double* t : {tm, tM}) CALLCHK(c, hipMemsetAsync(t, 0, (u64)n_loci * 8, st));
    const QModel* use = mdl.model != 4u || mdl.gene ? &mdl : nullptr;
    for (u32 done = 0; done < n_reps;) {
        const u32 R = std::min<u32>(per, n_reps - done);
        // the batch's replicates as a CSC N of R columns
        u64 nnz_b = 0;
        if (p.W) RCCHK(bs_draw_batch(c, p, b, seed, done, R, nnz_b));
        DevBuf<> ec, cnt, locus, theta;
        CALLCHK(c, ec.alloc(std::max<u64>(nnz_b, 1) * 4));
        CALLCHK(c, cnt.alloc(std::max<u64>(nnz_b, 1) * 4));
        if (p.W) bs_emit(c, p, b, R, 0u, rep_ptr, ec.as<int>(), cnt.as<int>());
        else k_bs_fill_ptr<<<nblk((u64)R + 1, TPB), TPB, 0, st>>>(rep_ptr, (u64)R + 1, 0);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, hipStreamSynchronize(st));
        const QMat mb{m.n_ecs, n_loci, n_haps, m.nnz, m.ip, m.ix, m.da, R, nnz_b, rep_ptr, ec.as<int>(), cnt.as<int>()};
        // ... quantified as the cells of ecquant-cells: the support, then the EM (its refusals -- a malformed A, scale, the gene ids -- all
        // come in the first batch, before anything of the caller's is written)
        uint64_t ns = 0;
        RCCHK(qc_run(false, device, mb, nullptr, nullptr, nullptr, 0, 0.0, budget_bytes, 0, QcOut{cell_ptr, nullptr}, &ns));
        CALLCHK(c, locus.alloc(std::max<u64>(ns, 1) * 4));
        CALLCHK(c, theta.alloc(std::max<u64>(ns * n_haps, 1) * 8));
        const QcOut qo{cell_ptr, locus.p, theta.p, o.n_iter ? (u32*)o.n_iter + done : nullptr, o.delta ? (double*)o.delta + done : nullptr,
                       o.explained ? (long long*)o.explained + done : nullptr, o.converged ? (uint8_t*)o.converged + done : nullptr};
        RCCHK(qc_run(true, device, mb, nullptr, d_scale, nullptr, max_iters, tol, budget_bytes, ns, qo, nullptr, use));
        k_bs_moments<<<nblk(n_loci, TPB), TPB, 0, st>>>(cell_ptr, locus.as<int>(), theta.as<double>(), R, done, n_loci, n_haps, mm, MM, tm, tM,
                                                        o.reps ? (double*)o.reps + (u64)done * plane : nullptr);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, hipStreamSynchronize(st));          // (the batch's buffers go here)
        done += R;
    }
    k_bs_finish<<<nblk(plane, TPB), TPB, 0, st>>>(mm, MM, plane, n_reps, (double*)o.mean, (double*)o.sd);
    if (o.tot_mean && o.tot_sd) k_bs_finish<<<nblk(n_loci, TPB), TPB, 0, st>>>(tm, tM, n_loci, n_reps, (double*)o.tot_mean, (double*)o.tot_sd);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, hipStreamSynchronize(st));
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_resample_device(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                                   const void* d_data_n, int64_t sample, uint64_t seed, uint64_t b0, uint32_t n_reps, void* d_rep_ptr, void* d_rep_ec,
                                   void* d_rep_count, uint64_t capacity, uint64_t* nnz_out) {
    RCCHK(bs_check_resample(n_ecs, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, sample, b0, n_reps, d_rep_ptr));
    Call c(device, "ecboot: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    BsPlan p;
    RCCHK(bs_front(c, n_ecs, n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n, sample, p));
    int* ptr = c.get<int>((u64)n_reps + 1);            // (the caller's is written once the whole result stands)
    if (const int rc = c.missing()) return rc;
    const bool want = d_rep_ec && d_rep_count && capacity;
    struct Kept { DevBuf<> ec, cnt; u64 at = 0, n = 0; };
    std::vector<Kept> kept;
    u64 total = 0;
    if (!p.W || !n_reps) k_bs_fill_ptr<<<nblk((u64)n_reps + 1, TPB), TPB, 0, st>>>(ptr, (u64)n_reps + 1, 0);
    else {
        u32 per = 1;
        RCCHK(bs_batch_reps(c, p, 0, n_reps, per));
        BsBufs b;
        RCCHK(bs_bufs(c, p, per, b));
        for (u32 done = 0; done < n_reps;) {
            const u32 R = std::min<u32>(per, n_reps - done);
            u64 nnz_b = 0;
            RCCHK(bs_draw_batch(c, p, b, seed, (u32)(b0 + done), R, nnz_b));
            if (total + nnz_b >= (1ull << 31)) return fail(nullptr, ECB_ERR_LIMIT, "ecboot: the replicates hold 2^31 entries or more");
            Kept k;
            k.at = total; k.n = nnz_b;
            const bool keep = want && total + nnz_b <= capacity && nnz_b;
            if (keep) { CALLCHK(c, k.ec.alloc(nnz_b * 4)); CALLCHK(c, k.cnt.alloc(nnz_b * 4)); }
            bs_emit(c, p, b, R, (u32)total, ptr + done, keep ? k.ec.as<int>() : nullptr, keep ? k.cnt.as<int>() : nullptr);
            CALLCHK(c, hipGetLastError());
            CALLCHK(c, hipStreamSynchronize(st));      // (the table is the next batch's)
            if (keep) kept.push_back(std::move(k));
            total += nnz_b;
            done += R;
        }
    }
    CALLCHK(c, hipGetLastError());
    // the whole result stands: from here on the outputs are written
    CALLCHK(c, hipMemcpyAsync(d_rep_ptr, ptr, ((u64)n_reps + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (want && capacity >= total)
        for (const Kept& k : kept) {
            CALLCHK(c, hipMemcpyAsync((int*)d_rep_ec + k.at, k.ec.p, k.n * 4, hipMemcpyDeviceToDevice, st));
            CALLCHK(c, hipMemcpyAsync((int*)d_rep_count + k.at, k.cnt.p, k.n * 4, hipMemcpyDeviceToDevice, st));
        }
    CALLCHK(c, hipStreamSynchronize(st));
    if (nnz_out) *nnz_out = total;
    return ECB_OK;
}

extern "C" int ecb_resample(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
                            const int32_t* data_n, int64_t sample, uint64_t seed, uint64_t b0, uint32_t n_reps, int32_t* rep_ptr, int32_t* rep_ec,
                            int32_t* rep_count, uint64_t capacity, uint64_t* nnz_out) {
    RCCHK(bs_check_resample(n_ecs, n_samples, nnz_n, indptr_n, indices_n, data_n, sample, b0, n_reps, rep_ptr));
    Call c(device, "ecboot: "); if (c.rc) return c.rc;
    const bool want = rep_ec && rep_count && capacity;
    DevBuf<> ipn, ixn, dan, op, oe, oc;
    std::vector<StageIn> in = {{&ipn, indptr_n, ((u64)n_samples + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4},
                               {&op, nullptr, ((u64)n_reps + 1) * 4}};
    if (want) in.insert(in.end(), {{&oe, nullptr, capacity * 4}, {&oc, nullptr, capacity * 4}});
    RCCHK(stage_in(c, in));
    uint64_t total = 0;
    RCCHK(ecb_resample_device(device, n_ecs, n_samples, nnz_n, ipn.p, ixn.p, dan.p, sample, seed, b0, n_reps, op.p, oe.p, oc.p, want ? capacity : 0, &total));
    const u64 out = want && capacity >= total ? total * 4 : 0;
    RCCHK(stage_out(c, {{rep_ptr, &op, ((u64)n_reps + 1) * 4}, {rep_ec, &oe, out}, {rep_count, &oc, out}}));
    if (nnz_out) *nnz_out = total;
    return ECB_OK;
}

extern "C" int ecb_quantify_bootstrap_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* d_indptr_a,
                                             const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                             const void* d_indices_n, const void* d_data_n, int64_t sample, const void* d_scale, uint32_t max_iters,
                                             double tol, uint64_t budget_bytes, uint32_t n_genes, const void* d_gene, uint32_t model, uint64_t seed,
                                             uint32_t n_reps, void* d_mean, void* d_sd, void* d_tot_mean, void* d_tot_sd, void* d_reps, void* d_n_iter,
                                             void* d_delta, void* d_explained, void* d_converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, (const int*)d_indptr_a, (const int*)d_indices_a, (const int*)d_data_a,
                 n_samples, nnz_n, (const int*)d_indptr_n, (const int*)d_indices_n, (const int*)d_data_n};
    RCCHK(bs_check_boot(m, sample, tol, n_genes, d_gene, model, n_reps, d_mean, d_sd));
    return bs_boot_run(device, m, sample, d_scale, max_iters, tol, budget_bytes, QModel{model, n_genes, (const int*)d_gene}, seed, n_reps,
                       BsOut{d_mean, d_sd, d_tot_mean, d_tot_sd, d_reps, d_n_iter, d_delta, d_explained, d_converged});
}

extern "C" int ecb_quantify_bootstrap(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const int32_t* indptr_a,
                                      const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                                      const int32_t* indices_n, const int32_t* data_n, int64_t sample, const double* scale, uint32_t max_iters,
                                      double tol, uint64_t budget_bytes, uint32_t n_genes, const int32_t* gene, uint32_t model, uint64_t seed,
                                      uint32_t n_reps, double* mean, double* sd, double* tot_mean, double* tot_sd, double* reps, uint32_t* n_iter,
                                      double* delta, int64_t* explained, uint8_t* converged) {
    const QMat m{n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n};
    RCCHK(bs_check_boot(m, sample, tol, n_genes, gene, model, n_reps, mean, sd));
    Call c(device, "ecboot: "); if (c.rc) return c.rc;
    const u64 plane = (u64)n_haps * n_loci * 8, line = (u64)n_loci * 8, B = n_reps;
    const bool tot = tot_mean && tot_sd;
    QStage b;
    DevBuf<> sc, gn, om, os, otm, ots, orp, oit, odl, oex, ocv;
    std::vector<StageIn> in = q_stage(b, m);
    in.insert(in.end(), {{&om, nullptr, plane}, {&os, nullptr, plane}});
    if (scale) in.push_back({&sc, scale, plane});
    if (gene) in.push_back({&gn, gene, (u64)n_loci * 4});
    if (tot) in.insert(in.end(), {{&otm, nullptr, line}, {&ots, nullptr, line}});
    if (reps) in.push_back({&orp, nullptr, B * plane});
    if (n_iter) in.push_back({&oit, nullptr, B * 4});
    if (delta) in.push_back({&odl, nullptr, B * 8});
    if (explained) in.push_back({&oex, nullptr, B * 8});
    if (converged) in.push_back({&ocv, nullptr, B});
    RCCHK(stage_in(c, in));
    RCCHK(bs_boot_run(device, q_staged(b, m), sample, sc.p, max_iters, tol, budget_bytes, QModel{model, n_genes, gn.as<int>()}, seed, n_reps,
                      BsOut{om.p, os.p, otm.p, ots.p, orp.p, oit.p, odl.p, oex.p, ocv.p}));
    return stage_out(c, {{mean, &om, plane}, {sd, &os, plane}, {tot_mean, &otm, tot ? line : 0}, {tot_sd, &ots, tot ? line : 0},
                         {reps, &orp, reps ? B * plane : 0}, {n_iter, &oit, n_iter ? B * 4 : 0}, {delta, &odl, delta ? B * 8 : 0},
                         {explained, &oex, explained ? B * 8 : 0}, {converged, &ocv, converged ? B : 0}});
}
