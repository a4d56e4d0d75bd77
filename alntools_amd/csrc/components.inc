// ---- ecclusters: the connected components of the target-EC incidence (ecb_components / ecb_components_device; included by ecb.hip after
// boot.inc) ---------------------------------------------------------------------------------------------------------------------------------------
// The graph is on the T loci; the members of a row (its columns whose mask is not 0) are joined when the row links: w[e] >= min_count, w as
// count-alignments weighs it (k_ca_weights), and at least one member.  A lock-free union-find over u32 parent[T], in a fixed number of
// launches, no host loop that waits for a fixed point.
// The one invariant: parent[x] <= x, and a word of parent only ever falls.  k_cc_init writes parent[x] = x; after it every write is an
// atomicCAS or an atomicMin that stores a smaller value (a plain store could put back a larger one that another lane has since lowered).
//   - Every value a word has held is an ancestor of x in the forest, and stays one: a link is only ever replaced by a link to an ancestor
//     further up (path splitting), and a root is hooked below a smaller locus of the other tree.  So the root of a tree is its smallest
//     locus, a walk x -> parent[x] -> ... strictly descends and ends after fewer than T steps whatever else runs, and the numbering by root
//     below is the numbering by smallest locus.
//   - Hooks are device-scope atomicCAS(&parent[hi], hi, lo) on a ROOT hi, lo < hi a locus of the other tree: it succeeds only while hi still
//     is a root, so no link is ever lost; the lane that loses goes on from the value the CAS handed back (each loss is another lane's
//     progress).  Both sides are walked up before anything is hooked and no atomic is issued once they meet (cc_unite): on real data nearly
//     every union after the first few is such a no-op, and a star would otherwise queue up on one word.
//   - The eight XCDs have L2s of their own, and a plain load of parent may return an older value.  parent is read with relaxed agent-scope
//     atomic loads (cc_load).  Were a value stale all the same it would be harmless: an old ancestor is still an ancestor, the walk only
//     takes longer, and whether a locus is a root is decided by the CAS alone, at the memory side.
// Steps: k_ca_weights | k_gm_check<true> || read back (count-alignments' checks and refusals) || [zero masks present: k_ca_nonzero,
// k_scan_lb] | k_cc_init | k_cc_hook: one thread per CC_ITEMS non-zeros of A, never one per row -- a member is joined with the member before
// it in its row; the row is found as k_ca_keys finds it.  With a mask of 0 somewhere (GM_SAW_ZERO) the member before is found by bisecting
// the prefix sums of "has a mask" inside the row; without, it is the entry before and nothing walks | k_cc_flatten: every locus to its
// root, root flags | k_scan_lb: the roots numbered in ascending order | k_cc_loci: comp_of_locus, loci per component | k_cc_rows:
// comp_of_ec, linking rows and reads per component | k_cc_sizes || read back.
// The per-component sums are integer atomics (exact in any order): the lanes of a wave that share the component of its first waiting lane
// (two rounds of it), and then the waves of a workgroup of CC_SUM_TPB that found the same component, send one add (cc_group_add) -- a giant
// component is one address, and every row's own add to it would queue up there.
namespace {
constexpr u32 CC_ITEMS = 4;                          // k_cc_hook: non-zeros per thread
constexpr u32 CC_WG_ITEMS = TPB * CC_ITEMS;          // ... and per workgroup
constexpr u32 CC_SUM_TPB = 1024;                     // k_cc_loci, k_cc_rows, k_cc_sizes: threads (a workgroup's adds to one component become one)
constexpr u32 CC_AGG_ROUNDS = 2;                     // ... and rounds of wave aggregation before the lanes left add on their own
static_assert(CC_ITEMS == 4, "k_cc_hook loads its columns as one uint4");

__device__ __forceinline__ u32 cc_load(const u32* parent, u32 x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the root of x, every locus passed on the way pointed at its grandparent (path splitting; atomicMin: the word only falls)
__device__ __forceinline__ u32 cc_find(u32* parent, u32 x) {
    u32 p = cc_load(parent, x);
    while (p != x) {
        const u32 g = cc_load(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p; p = g;
    }
    return x;
}
// a and b into one tree.  Both walks go up together, the side whose parent is the larger one a step at a time (Rem's order), and stop as
// soon as the two parents are equal: a common ancestor, so one tree already, and no atomic is issued.  In a component that has formed,
// nearly every locus points at the root, and such a union is two loads at two places of their own -- the root's word, which every find of
// a giant component would read, is not touched.  A side that is a root above the other side's parent is hooked below it (pb may be an older
// parent of b: still a locus of b's tree, and below a); a lost CAS hands back the word's new value and the walk goes on from there.
__device__ __forceinline__ void cc_unite(u32* parent, u32 a, u32 b) {
    u32 pa = cc_load(parent, a), pb = cc_load(parent, b);
    while (pa != pb) {
        if (pa < pb) { u32 t = a; a = b; b = t; t = pa; pa = pb; pb = t; }      // a's parent is the larger one
        if (pa == a) {
            const u32 old = atomicCAS(parent + a, a, pb);
            if (old == a) return;
            pa = old;
        } else {
            const u32 g = cc_load(parent, pa);
            if (g != pa) atomicMin(parent + a, g);                             // (path splitting, as in cc_find)
            a = pa; pa = g;
        }
    }
}
// the last j of [lo, hi) with excl[j] < v (there is one: excl[lo] < v)
__device__ __forceinline__ u64 cc_last_below(const u32* excl, u64 lo, u64 hi, u32 v) {
    while (lo + 1 < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (excl[mid] < v) lo = mid; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(TPB) void k_cc_init(u32* parent, u32 n_loci) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t < n_loci) parent[t] = (u32)t;
}
// thread k of workgroup b: non-zeros [b CC_WG_ITEMS + 4k, + 4) of A.  ZERO: a mask of 0 was seen, nz_excl = the exclusive prefix sums of
// "non-zero i has a mask" (nnz + 1 values)
template <bool ZERO>
__global__ __launch_bounds__(TPB) void k_cc_hook(const int* indptr, u32 n_ecs, const int* indices, u64 nnz, const u64* ww, u64 min_count,
                                                 const u32* nz_excl, u32* parent) {
    __shared__ u32 s_row[2];
    const u64 b0 = blockIdx.x * (u64)CC_WG_ITEMS, b1 = std::min<u64>(nnz, b0 + CC_WG_ITEMS) - 1;
    ca_block_rows(indptr, n_ecs, b0, b1, s_row);
    const u64 i0 = b0 + (u64)threadIdx.x * CC_ITEMS;
    if (i0 >= nnz) return;
    const u32 hi = s_row[1];
    u32 c[CC_ITEMS];
    if (i0 + CC_ITEMS <= nnz && (reinterpret_cast<uintptr_t>(indices) & 15u) == 0u) {
        const uint4 q = reinterpret_cast<const uint4*>(indices + i0)[0];
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
        for (u32 j = 0; j < CC_ITEMS; ++j) c[j] = i0 + j < nnz ? (u32)indices[i0 + j] : 0u;
    }
    u32 prev = i0 ? (u32)indices[i0 - 1] : 0u;
    u32 r = ca_row_of(indptr, s_row[0], hi, i0);
    bool links = (ww[r] & CA_WEIGHT) >= min_count;
#pragma unroll
    for (u32 j = 0; j < CC_ITEMS; ++j) {
        const u64 i = i0 + j;
        if (i >= nnz) break;
        if (r < hi && (u64)(u32)indptr[r + 1] <= i) { r = ca_row_of(indptr, r + 1, hi, i); links = (ww[r] & CA_WEIGHT) >= min_count; }
        const u64 a = (u64)(u32)indptr[r];
        if (links && i > a) {
            if (!ZERO) cc_unite(parent, c[j], prev);
            else if (nz_excl[i + 1] != nz_excl[i] && nz_excl[i] != nz_excl[a])      // a member, and not its row's first
                cc_unite(parent, c[j], (u32)indices[cc_last_below(nz_excl, a, i, nz_excl[i])]);
        }
        prev = c[j];
    }
}
// locus t: its root, and whether it is one
__global__ __launch_bounds__(TPB) void k_cc_flatten(u32* parent, u32 n_loci, u32* root, u32* flag) {
    const u64 t = blockIdx.x * (u64)TPB + threadIdx.x;
    if (t >= n_loci) return;
    const u32 r = cc_find(parent, (u32)t);
    root[t] = r;
    flag[t] = r == (u32)t;
}
// every thread of the workgroup calls this (valid: this thread has something to add to component comp): cnt[comp] += n and, sum not null,
// sum[comp] += v.  CC_AGG_ROUNDS times, the lanes of a wave that share the component of its first waiting lane become one (component, n, v)
// -- the second round, because the first waiting lane of a wave need not sit in the component most of its lanes sit in --; a lane still
// waiting then adds on its own.  Thread 0 adds up what the waves found for the workgroup's heaviest component and sends it as one add of
// each; the rest go as they are.
__device__ __forceinline__ void cc_group_add(int* cnt, long long* sum, u32 comp, bool valid, u32 n, u64 v) {
    constexpr u32 SLOTS = CC_SUM_TPB / 64 * CC_AGG_ROUNDS;
    __shared__ u32 s_c[SLOTS], s_n[SLOTS];
    __shared__ u64 s_v[SLOTS];
    const u32 lane = threadIdx.x & 63u;
    u64 left = __ballot(valid);
#pragma unroll
    for (u32 r = 0; r < CC_AGG_ROUNDS; ++r) {
        const int lead = left ? __ffsll((long long)left) - 1 : 0;
        const u32 lc = (u32)__builtin_amdgcn_readlane((int)comp, lead);
        const bool same = ((left >> lane) & 1ull) && comp == lc;
        const u32 ns = wave_sum(same ? n : 0u);
        u64 vs = same ? v : 0ull;
        if (sum) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) vs += __shfl_xor(vs, d);
        }
        if (lane == 0u) { const u32 k = (threadIdx.x >> 6) * CC_AGG_ROUNDS + r; s_c[k] = lc; s_n[k] = ns; s_v[k] = vs; }
        left &= ~__ballot(same);
    }
    if ((left >> lane) & 1ull) {
        if (n) atomicAdd(cnt + comp, (int)n);
        if (sum && v) atomicAdd(reinterpret_cast<unsigned long long*>(sum + comp), (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u32 best = 0;
    for (u32 k = 1; k < SLOTS; ++k) if (s_n[k] > s_n[best]) best = k;
    const u32 c = s_c[best];
    u32 nn = 0;
    u64 vv = 0;
    for (u32 k = 0; k < SLOTS; ++k) {
        if (!s_n[k] && !s_v[k]) continue;                               // (a round with nothing to add)
        if (s_c[k] == c) { nn += s_n[k]; vv += s_v[k]; continue; }
        if (s_n[k]) atomicAdd(cnt + s_c[k], (int)s_n[k]);
        if (sum && s_v[k]) atomicAdd(reinterpret_cast<unsigned long long*>(sum + s_c[k]), (unsigned long long)s_v[k]);
    }
    if (nn) atomicAdd(cnt + c, (int)nn);
    if (sum && vv) atomicAdd(reinterpret_cast<unsigned long long*>(sum + c), (unsigned long long)vv);
}
// locus t: its component = the number of roots below its root (excl: the exclusive prefix sums of the root flags)
__global__ __launch_bounds__(CC_SUM_TPB) void k_cc_loci(const u32* root, const u32* excl, u32 n_loci, int* comp_of_locus, int* comp_loci) {
    const u64 t = blockIdx.x * (u64)CC_SUM_TPB + threadIdx.x;
    const bool valid = t < n_loci;
    u32 comp = 0;
    if (valid) { comp = excl[root[t]]; comp_of_locus[t] = (int)comp; }
    cc_group_add(comp_loci, nullptr, comp, valid, 1u, 0ull);
}
// row e: whether it links, and then the component of its first member
__global__ __launch_bounds__(CC_SUM_TPB) void k_cc_rows(const int* indptr, u32 n_ecs, const int* indices, const u64* ww, u64 min_count,
                                                        const u32* nz_excl, const int* comp_of_locus, int* comp_of_ec, int* comp_ecs,
                                                        long long* comp_reads) {
    const u64 e = blockIdx.x * (u64)CC_SUM_TPB + threadIdx.x;
    bool links = false;
    u32 comp = 0;
    u64 w = 0;
    if (e < n_ecs) {
        const u64 a = (u64)(u32)indptr[e], b = (u64)(u32)indptr[e + 1];
        w = ww[e] & CA_WEIGHT;
        u64 first = a;
        bool member = b > a;
        if (member && nz_excl) {
            member = nz_excl[b] != nz_excl[a];
            if (member) first = cc_last_below(nz_excl, a, b + 1, nz_excl[a] + 1u);      // (the last j whose prefix still is the row's: the first member)
        }
        links = member && w >= min_count;
        if (links) comp = (u32)comp_of_locus[(u32)indices[first]];
        if (comp_of_ec) comp_of_ec[e] = links ? (int)comp : -1;
    }
    cc_group_add(comp_ecs, comp_reads, comp, links, 1u, w);
}
// words[3] = the linking rows (the sum of comp_ecs: a count of its own in k_cc_rows was one add per wave to one word, 0.7 ms at 3.7 M
// rows), words[4] = the loci of the largest component, words[5] = the components of two loci or more; three adds per workgroup
__global__ __launch_bounds__(CC_SUM_TPB) void k_cc_sizes(const int* comp_loci, const int* comp_ecs, u32 n_loci, u64* words) {
    __shared__ u32 s_big[CC_SUM_TPB / 64], s_multi[CC_SUM_TPB / 64], s_link[CC_SUM_TPB / 64];
    const u64 t = blockIdx.x * (u64)CC_SUM_TPB + threadIdx.x;
    const u32 n = t < n_loci ? (u32)comp_loci[t] : 0u;
    const u32 multi = wave_sum(n >= 2u ? 1u : 0u), link = wave_sum(t < n_loci ? (u32)comp_ecs[t] : 0u);      // (the rows are fewer than 2^31)
    u32 big = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) big = std::max(big, (u32)__shfl_xor((int)big, d));
    if ((threadIdx.x & 63u) == 0u) { s_big[threadIdx.x >> 6] = big; s_multi[threadIdx.x >> 6] = multi; s_link[threadIdx.x >> 6] = link; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 b = 0, m = 0, l = 0;
    for (u32 k = 0; k < CC_SUM_TPB / 64; ++k) { b = std::max<u64>(b, s_big[k]); m += s_multi[k]; l += s_link[k]; }
    if (l) atomicAdd(reinterpret_cast<unsigned long long*>(words + 3), (unsigned long long)l);
    if (b) atomicMax(reinterpret_cast<unsigned long long*>(words + 4), (unsigned long long)b);
    if (m) atomicAdd(reinterpret_cast<unsigned long long*>(words + 5), (unsigned long long)m);
}
// what both entry points refuse before anything is allocated
int cc_check_args(uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a, const void* indptr_a, const void* indices_a, const void* data_a,
                  uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, int64_t sample, int64_t min_count,
                  const void* comp_of_locus, const void* out_sizes) {
    if (!comp_of_locus || !out_sizes) return fail(nullptr, ECB_ERR_ARG, "components: bad argument (no comp_of_locus, or no out_sizes)");
    if (min_count < 0) return fail(nullptr, ECB_ERR_ARG, "components: a negative min_count (%lld)", (long long)min_count);
    return ca_check_args(n_ecs, n_loci, n_haps, nnz_a, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n, sample);
}
}  // namespace

extern "C" int ecb_components_device(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const void* d_indptr_a,
                                     const void* d_indices_a, const void* d_data_a, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n,
                                     const void* d_indices_n, const void* d_data_n, int64_t sample, int64_t min_count, void* d_comp_of_locus,
                                     void* d_comp_of_ec, void* d_comp_loci, void* d_comp_ecs, void* d_comp_reads, uint64_t* out_sizes) {
    RCCHK(cc_check_args(n_ecs, n_loci, n_haps, nnz, d_indptr_a, d_indices_a, d_data_a, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, sample,
                        min_count, d_comp_of_locus, out_sizes));
    Call c(device, "components: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 T = n_loci;
    // apply-mask's words; [1] the error bits of N, [2] a scan's total (the entries with a mask, then the components), [3] the linking rows,
    // [4] the largest component, [5] the components of two loci or more
    const u64 n_words = GM_SHARD_WORDS * (1 + GM_SHARDS);
    u64* words = c.get<u64>(CV_WORDS, n_words);
    u32 *bits = c.get<u32>(CV_X0, nnz), *sums = c.get<u32>(CV_SUMS2, scan_words(std::max<u64>(nnz, T)));
    u64* ww = c.get<u64>(CV_X2, n_ecs);
    u32 *parent = c.get<u32>(CV_X3, T), *root = c.get<u32>(CV_VALS0, T), *flag = c.get<u32>(CV_VALS1, T), *excl = c.get<u32>(CV_SCAN, T + 1);
    int* loci = d_comp_loci ? (int*)d_comp_loci : c.get<int>(CV_HEAD, T);
    int* ecs = d_comp_ecs ? (int*)d_comp_ecs : c.get<int>(CV_BLK, T);
    long long* reads = d_comp_reads ? (long long*)d_comp_reads : c.get<long long>(CV_KEYS0, T);
    if (const int rc = c.missing()) return rc;
    const int* ip = (const int*)d_indptr_a; const int* ix = (const int*)d_indices_a; const int* da = (const int*)d_data_a;
    CALLCHK(c, hipMemsetAsync(words, 0, n_words * 8, st));
    CALLCHK(c, hipMemsetAsync(ww, 0, std::max<u64>(n_ecs, 1) * 8, st));
    k_ca_weights<<<nblk(std::max<u64>(nnz_n, (u64)n_samples + 1), TPB), TPB, 0, st>>>((const int*)d_indptr_n, n_samples, (const int*)d_indices_n,
                                                                                     (const int*)d_data_n, nnz_n, n_ecs, sample, ww, words);
    k_gm_check<true><<<nblk(std::max<u64>((u64)n_ecs + 1, (nnz + GM_ITEMS - 1) / GM_ITEMS), TPB), TPB, 0, st>>>(ip, n_ecs, ix, da, nnz, nullptr, n_loci,
                                                                                                             n_haps, bits, words);
    CALLCHK(c, hipGetLastError());
    std::vector<u64> back(n_words);
    if (const int rc = c.read_back(back.data(), words, n_words, GM_ERRS)) return rc;
    RCCHK(ca_refuse_input(back));
    // the input is well formed: from here on the outputs are written
    u32* nz_excl = nullptr;
    if ((u32)back[0] & GM_SAW_ZERO) {
        nz_excl = c.get<u32>(CV_X1, nnz + 1);
        if (const int rc = c.missing()) return rc;
        k_ca_nonzero<<<nblk(nnz, TPB), TPB, 0, st>>>(bits, nnz);
        CALLCHK(c, scan_launch(st, bits, nnz, nz_excl, sums, words + 2, 1, nz_excl + nnz));
    }
    const u64 least = (u64)min_count;
    k_cc_init<<<nblk(T, TPB), TPB, 0, st>>>(parent, n_loci);
    if (nnz) {
        if (nz_excl) k_cc_hook<true><<<nblk(nnz, CC_WG_ITEMS), TPB, 0, st>>>(ip, n_ecs, ix, nnz, ww, least, nz_excl, parent);
        else k_cc_hook<false><<<nblk(nnz, CC_WG_ITEMS), TPB, 0, st>>>(ip, n_ecs, ix, nnz, ww, least, nullptr, parent);
    }
    k_cc_flatten<<<nblk(T, TPB), TPB, 0, st>>>(parent, n_loci, root, flag);
    CALLCHK(c, hipGetLastError());
    CALLCHK(c, scan_launch(st, flag, T, excl, sums, words + 2, 1, excl + T));
    CALLCHK(c, hipMemsetAsync(loci, 0, T * 4, st));
    CALLCHK(c, hipMemsetAsync(ecs, 0, T * 4, st));
    CALLCHK(c, hipMemsetAsync(reads, 0, T * 8, st));
    k_cc_loci<<<nblk(T, CC_SUM_TPB), CC_SUM_TPB, 0, st>>>(root, excl, n_loci, (int*)d_comp_of_locus, loci);
    if (n_ecs) k_cc_rows<<<nblk(n_ecs, CC_SUM_TPB), CC_SUM_TPB, 0, st>>>(ip, n_ecs, ix, ww, least, nz_excl, (const int*)d_comp_of_locus, (int*)d_comp_of_ec, ecs, reads);
    k_cc_sizes<<<nblk(T, CC_SUM_TPB), CC_SUM_TPB, 0, st>>>(loci, ecs, n_loci, words);
    CALLCHK(c, hipGetLastError());
    u64 out[6];
    if (const int rc = c.read_back(out, words, 6)) return rc;
    out_sizes[0] = out[2]; out_sizes[1] = out[3]; out_sizes[2] = out[4]; out_sizes[3] = out[5];
    return ECB_OK;
}

extern "C" int ecb_components(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz, const int32_t* indptr_a,
                              const int32_t* indices_a, const int32_t* data_a, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n,
                              const int32_t* indices_n, const int32_t* data_n, int64_t sample, int64_t min_count, int32_t* comp_of_locus,
                              int32_t* comp_of_ec, int32_t* comp_loci, int32_t* comp_ecs, int64_t* comp_reads, uint64_t* out_sizes) {
    RCCHK(cc_check_args(n_ecs, n_loci, n_haps, nnz, indptr_a, indices_a, data_a, n_samples, nnz_n, indptr_n, indices_n, data_n, sample, min_count,
                        comp_of_locus, out_sizes));
    Call c(device, "components: "); if (c.rc) return c.rc;
    const u64 T = n_loci;
    DevBuf<> ipa, ixa, daa, ipn, ixn, dan, ol, oe, cl, ce, cr;
    std::vector<StageIn> in = {{&ipa, indptr_a, ((u64)n_ecs + 1) * 4}, {&ixa, indices_a, nnz * 4}, {&daa, data_a, nnz * 4},
                               {&ipn, indptr_n, ((u64)n_samples + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4},
                               {&ol, nullptr, T * 4}};
    if (comp_of_ec) in.push_back({&oe, nullptr, (u64)n_ecs * 4});
    if (comp_loci) in.push_back({&cl, nullptr, T * 4});
    if (comp_ecs) in.push_back({&ce, nullptr, T * 4});
    if (comp_reads) in.push_back({&cr, nullptr, T * 8});
    int rc = stage_in(c, in);
    if (rc == ECB_OK) rc = ecb_components_device(device, n_ecs, n_loci, n_haps, nnz, ipa.p, ixa.p, daa.p, n_samples, nnz_n, ipn.p, ixn.p, dan.p, sample,
                                                 min_count, ol.p, oe.p, cl.p, ce.p, cr.p, out_sizes);
    RCCHK(rc);
    return stage_out(c, {{comp_of_locus, &ol, T * 4}, {comp_of_ec, &oe, comp_of_ec ? (u64)n_ecs * 4 : 0}, {comp_loci, &cl, comp_loci ? T * 4 : 0},
                         {comp_ecs, &ce, comp_ecs ? T * 4 : 0}, {comp_reads, &cr, comp_reads ? T * 8 : 0}});
}
