// ---- ecdownsample: n of a sample's M reads kept, drawn without replacement (ecb_downsample / ecb_downsample_device; included by ecb.hip
// behind umi.inc, ds_key.h before it; Call, Arena, the scan, the check of N and the per-sample totals are ecb.hip's) ----------------------
// The rule is include/ecb_downsample.h's: the n_s reads of sample s with the smallest 128-bit keys ds_key(seed, s, r) stay.  No key is ever
// stored: every pass regenerates the keys it looks at (ten Philox rounds cost less than 16 bytes of memory traffic per read).  The
// selection is an MSB-first radix select on the key's sixteen 8-bit digits: the histogram of digit d over the reads whose first d digits
// are the prefix fixed so far names the bin b that holds the n-th smallest key; the bins below b stay, the bins above go, and the select
// goes on inside b with what is still to take -- until the bin is taken whole ("resolved").  Keys of one sample never tie, so the last
// digit's bins hold one read each and resolve at the latest.  What a resolved sample leaves is (prefix, depth): a read stays iff the
// first depth + 1 digits of its key, read as one number, are at most the prefix's.
// Steps: k_sel_ncheck, k_sel_totals (ecselect's: N checked, M_s), k_ds_plan (a mode per sample), two scans (the large samples numbered,
// their stretches numbered) || read back: refusals; from here on the outputs are written || no sample thinned or emptied: a copy.  Otherwise
// k_ds_init (the copied columns copied, every other count 0), then per mode:
//   small (M_s <= DS_SMALL): k_ds_small, one workgroup per sample.  The keys of its reads sit in registers (DS_SMALL_READS per thread),
//     the histogram in LDS, the digits are taken in a loop until the sample resolves, the counts are added up in LDS and stored by the
//     same workgroup: nothing per sample lives in global memory but the output.
//   large: a DsState and a 256-word histogram per sample in global memory (at most total reads / DS_SMALL of them: half a byte of
//     histogram per read).  The reads of a large sample are dealt to workgroups in stretches of DS_WG_READS consecutive reads, a thread
//     DS_THREAD_READS consecutive ones, whatever the entries' counts are (a pass over keys does not look at the entries at all).
//     Pass d: k_ds_hist -- a read whose key has the sample's prefix adds 1 to bin digit(d) in LDS, the workgroup flushes with at most 256
//     global adds -- then k_ds_pick, one workgroup per sample: the bin, the new prefix, resolved or not.  || read back one word, the
//     samples still unresolved; 0 ends the loop (16 passes at the most).  k_ds_count: a thread finds the entry of its first read by
//     bisection in the exclusive prefix sums of the counts, walks (a bisection again where an entry ends), adds up a run of reads of one
//     entry in a register, and a wave whose lanes all ended in one entry sends one add.
namespace {
constexpr u32 DS_SMALL = 2048;                                 // a sample of at most this many reads is one workgroup's (k_ds_small)
constexpr u32 DS_SMALL_READS = DS_SMALL / TPB;                 // keys a thread of k_ds_small holds in registers: read tid + i TPB
constexpr u32 DS_THREAD_READS = 16;                            // consecutive reads per thread of k_ds_hist / k_ds_count
constexpr u32 DS_WAVE_READS = 64 * DS_THREAD_READS;            // ... per wave
constexpr u32 DS_WG_READS = TPB * DS_THREAD_READS;             // ... per workgroup: a stretch
constexpr u32 DS_BINS = 256;                                   // bins of a digit
constexpr u32 DS_DIGITS = 16;                                  // digits of a key
constexpr u64 DS_MAX_READS = 1ull << 31;                       // a read's number is one counter word: M_s below this for a thinned sample
constexpr u64 DS_MAX_STRETCHES = 1ull << 31;                   // the grid of a pass over the large samples
enum : u32 { DS_COPY = 0, DS_ZERO, DS_SMALL_MODE, DS_LARGE_MODE };
// status words: [1] the error bits of N  [2] a thinned sample of 2^31 reads or more  [3] samples thinned in k_ds_small  [4] large samples
// (a scan's total)  [5] their stretches (a scan's total)  [6] large samples still unresolved after a pass  [7] samples that are not copied
enum : u32 { DS_W_ERR = 1, DS_W_LIMIT, DS_W_SMALL, DS_W_LARGE, DS_W_STRETCHES, DS_W_OPEN, DS_W_CHANGED, DS_WORDS };
static_assert(DS_WORDS == 8, "the status words");
static_assert(DS_BINS == (u32)TPB, "a histogram is one bin per thread of a workgroup (k_ds_small, k_ds_hist, k_ds_pick)");
static_assert(DS_SMALL == DS_SMALL_READS * (u32)TPB && DS_SMALL_READS >= 1u, "k_ds_small holds every key of a small sample in registers");
static_assert(DS_SMALL < (1u << 16), "k_ds_small scans reads and non-zero entries in one word: 16 bits each");
static_assert(DS_WG_READS == 4u * DS_WAVE_READS && DS_WG_READS >= DS_SMALL, "a stretch is four waves' reads, and a large sample fills at least half of its last one on average");
static_assert(8u * DS_DIGITS == 128u && DS_BINS == 256u, "sixteen 8-bit digits");

struct DsState { DsKey pfx; u32 need, depth, resolved, sample, reads, pad[3]; };      // a large sample: 48 bytes
static_assert(sizeof(DsState) == 48, "DsState");

// inclusive sum over the workgroup (s_w: TPB / 64 words; two barriers, the second one frees s_w); *total: the workgroup's sum
__device__ __forceinline__ u32 ds_block_incl(u32 v, u32* s_w, u32* total) {
    const u32 incl = wave_incl_scan(v), w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_w[w] = incl;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < (u32)TPB / 64u; ++k) { const u32 c = s_w[k]; if (k < w) before += c; tot += c; }
    __syncthreads();
    *total = tot;
    return before + incl;
}
// the bin b of a histogram (h: this thread's bin) with below < need <= below + h[b]: s_sel = {b, below, need == below + h[b]}.
// need is at least 1 and at most the histogram's sum, so exactly one thread writes
__device__ __forceinline__ void ds_pick_bin(u32 h, u32 need, u32* s_w, u32* s_sel) {
    u32 tot;
    const u32 incl = ds_block_incl(h, s_w, &tot), below = incl - h;
    if (below < need && need <= incl) { s_sel[0] = threadIdx.x; s_sel[1] = below; s_sel[2] = need == incl; }
    __syncthreads();
}

// sample s: its mode, the reads it keeps (otot), whether it is large and how many stretches it then has
__global__ __launch_bounds__(TPB) void k_ds_plan(const u64* tot, const long long* target, u32 n_samples, u32* mode, long long* otot, u32* large,
                                                 u32* stretches, u64* words) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s >= n_samples) return;
    const u64 M = tot[s];
    const long long n = target[s];
    u32 m = DS_COPY;
    if (n >= 0 && (u64)n < M) {
        if (M >= DS_MAX_READS) atomicOr(reinterpret_cast<u32*>(words + DS_W_LIMIT), 1u);
        m = n == 0 ? DS_ZERO : M <= DS_SMALL ? DS_SMALL_MODE : DS_LARGE_MODE;
    }
    mode[s] = m;
    otot[s] = m == DS_COPY ? (long long)M : n;
    large[s] = m == DS_LARGE_MODE;
    stretches[s] = m == DS_LARGE_MODE ? (u32)((std::min<u64>(M, DS_MAX_READS) + DS_WG_READS - 1u) / DS_WG_READS) : 0u;
    if (m == DS_SMALL_MODE) atomicAdd(reinterpret_cast<unsigned long long*>(words + DS_W_SMALL), 1ull);
    if (m != DS_COPY) atomicAdd(reinterpret_cast<unsigned long long*>(words + DS_W_CHANGED), 1ull);
}
// thread t: entries [4t, 4t + 4) of N: a copied column's counts as they are, every other count 0 (the thinned ones are added up later)
__global__ __launch_bounds__(SEL_TPB) void k_ds_init(const int* indptr_n, u32 n_samples, const int* data_n, u64 nnz_n, const u32* mode, int* out) {
    __shared__ u32 s_col[2];
    const u64 b0 = blockIdx.x * (u64)(SEL_TPB * SEL_ITEMS), b1 = std::min<u64>(nnz_n, b0 + SEL_TPB * SEL_ITEMS) - 1;
    ca_block_rows(indptr_n, n_samples, b0, b1, s_col);
    const u64 i0 = b0 + (u64)threadIdx.x * SEL_ITEMS;
    if (i0 >= nnz_n) return;
    const u32 hi = s_col[1];
    u32 col = ca_row_of(indptr_n, s_col[0], hi, i0);
#pragma unroll
    for (u32 j = 0; j < SEL_ITEMS; ++j) {
        const u64 i = i0 + j;
        if (i >= nnz_n) break;
        if (col < hi && (u64)(u32)indptr_n[col + 1] <= i) col = ca_row_of(indptr_n, col + 1, hi, i);
        out[i] = mode[col] == DS_COPY ? data_n[i] : 0;
    }
}
// workgroup s: a small sample thinned.  s_start[p]: the first read of the column's p-th entry that has reads, s_idx[p]: that entry's
// place in the column, s_cnt[p]: its reads that stay
__global__ __launch_bounds__(TPB) void k_ds_small(const int* indptr_n, const int* data_n, const u32* mode, const long long* target, u64 seed, int* out) {
    __shared__ u32 s_start[DS_SMALL + 1], s_idx[DS_SMALL], s_cnt[DS_SMALL], s_hist[DS_BINS], s_w[TPB / 64], s_sel[3];
    const u32 s = blockIdx.x, tid = threadIdx.x;
    if (mode[s] != DS_SMALL_MODE) return;
    const u32 a = (u32)indptr_n[s], b = (u32)indptr_n[s + 1];
    u32 run = 0;                                     // reads | entries with reads << 16, of the entries before this round's
    for (u32 base = a; base < b; base += TPB) {
        const u32 j = base + tid, c = j < b ? (u32)data_n[j] : 0u, v = c | (c ? 1u << 16 : 0u);
        u32 tot;
        const u32 excl = run + ds_block_incl(v, s_w, &tot) - v;
        if (c) { const u32 p = excl >> 16; s_start[p] = excl & 0xFFFFu; s_idx[p] = j - a; s_cnt[p] = 0u; }
        run += tot;
    }
    const u32 M = run & 0xFFFFu, nz = run >> 16;
    if (tid == 0) s_start[nz] = M;
    // the keys; what[i]: 0 = still in the bin the select is in, 1 = stays, 2 = goes
    DsKey key[DS_SMALL_READS];
    u32 what[DS_SMALL_READS];
#pragma unroll
    for (u32 i = 0; i < DS_SMALL_READS; ++i) {
        const u32 r = tid + i * TPB;
        what[i] = r < M ? 0u : 2u;
        key[i] = ds_key(seed, s, r);
    }
    u32 need = (u32)target[s];
    for (u32 d = 0; d < DS_DIGITS; ++d) {
        s_hist[tid] = 0u;
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < DS_SMALL_READS; ++i) if (what[i] == 0u) atomicAdd(&s_hist[ds_digit(key[i], d)], 1u);
        __syncthreads();
        ds_pick_bin(s_hist[tid], need, s_w, s_sel);
        const u32 bin = s_sel[0], below = s_sel[1], done = s_sel[2];
#pragma unroll
        for (u32 i = 0; i < DS_SMALL_READS; ++i) {
            if (what[i] != 0u) continue;
            const u32 g = ds_digit(key[i], d);
            what[i] = g < bin || (done && g == bin) ? 1u : g > bin ? 2u : 0u;
        }
        __syncthreads();                             // (s_sel and s_hist are the next round's)
        if (done) break;
        need -= below;
    }
#pragma unroll
    for (u32 i = 0; i < DS_SMALL_READS; ++i) {
        if (what[i] != 1u) continue;
        const u32 r = tid + i * TPB;
        u32 lo = 0, hi = nz - 1u;                    // the last p with s_start[p] <= r
        while (lo < hi) { const u32 mid = lo + (hi - lo + 1u) / 2u; if (s_start[mid] <= r) lo = mid; else hi = mid - 1u; }
        atomicAdd(&s_cnt[lo], 1u);
    }
    __syncthreads();
    for (u32 p = tid; p < nz; p += TPB) out[a + s_idx[p]] = (int)s_cnt[p];
}
// sample s, if it is large: its state and where its stretches start (stretch0[n_large]: their number)
__global__ __launch_bounds__(TPB) void k_ds_large_init(const u32* mode, const u32* lpos, const u32* spos, const u64* tot, const long long* target,
                                                       u32 n_samples, u32 n_large, u32 n_stretches, DsState* state, u32* stretch0) {
    const u64 s = blockIdx.x * (u64)TPB + threadIdx.x;
    if (s == 0) stretch0[n_large] = n_stretches;
    if (s >= n_samples || mode[s] != DS_LARGE_MODE) return;
    const u32 l = lpos[s];
    DsState st{};
    st.need = (u32)target[s]; st.sample = (u32)s; st.reads = (u32)tot[s];
    state[l] = st;
    stretch0[l] = spos[s];
}
// the large sample a workgroup's stretch lies in (every thread of the workgroup calls this) and the stretch's first read
__device__ __forceinline__ u32 ds_stretch_sample(const u32* stretch0, u32 n_large, u32* s_l, u32* first_read) {
    if (threadIdx.x == 0) {
        u32 lo = 0, hi = n_large - 1u;               // the last l with stretch0[l] <= blockIdx.x
        while (lo < hi) { const u32 mid = lo + (hi - lo + 1u) / 2u; if (stretch0[mid] <= blockIdx.x) lo = mid; else hi = mid - 1u; }
        *s_l = lo;
    }
    __syncthreads();
    const u32 l = *s_l;
    *first_read = (blockIdx.x - stretch0[l]) * DS_WG_READS;
    return l;
}
// pass d over a stretch of an unresolved large sample: hist[l][digit d] += the reads whose key has the sample's prefix
__global__ __launch_bounds__(TPB) void k_ds_hist(const u32* stretch0, u32 n_large, const DsState* state, u64 seed, u32 d, u32* hist) {
    __shared__ u32 s_hist[DS_BINS], s_l;
    u32 r0;
    const u32 l = ds_stretch_sample(stretch0, n_large, &s_l, &r0);
    const DsState st = state[l];
    if (st.resolved) return;
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    r0 += threadIdx.x * DS_THREAD_READS;
#pragma unroll 4
    for (u32 i = 0; i < DS_THREAD_READS; ++i) {
        const u32 r = r0 + i;
        if (r >= st.reads) break;
        const DsKey k = ds_key(seed, st.sample, r);
        if (ds_match(k, st.pfx, d)) atomicAdd(&s_hist[ds_digit(k, d)], 1u);
    }
    __syncthreads();
    const u32 h = s_hist[threadIdx.x];
    if (h) atomicAdd(hist + (u64)l * DS_BINS + threadIdx.x, h);
}
// workgroup l after pass d: the bin that holds the need-th smallest key of the prefix's bucket; the histogram zeroed for the next pass
__global__ __launch_bounds__(TPB) void k_ds_pick(DsState* state, u32* hist, u32 d, u64* words) {
    __shared__ u32 s_w[TPB / 64], s_sel[3];
    const u32 l = blockIdx.x;
    if (state[l].resolved) return;
    const u32 h = hist[(u64)l * DS_BINS + threadIdx.x], need = state[l].need;
    hist[(u64)l * DS_BINS + threadIdx.x] = 0u;
    __syncthreads();                                 // (every thread has read the state that thread 0 rewrites)
    ds_pick_bin(h, need, s_w, s_sel);
    if (threadIdx.x != 0) return;
    DsState st = state[l];
    ds_set_digit(st.pfx, d, s_sel[0]);
    st.depth = d;
    st.need = need - s_sel[1];
    st.resolved = s_sel[2];
    state[l] = st;
    if (!st.resolved) atomicAdd(reinterpret_cast<unsigned long long*>(words + DS_W_OPEN), 1ull);
}
// the last j of [lo, hi] with cum[j] - base <= r (cum: exclusive prefix sums over all entries, modulo 2^32; a thinned column's differences fit)
__device__ __forceinline__ u32 ds_entry_of(const u32* cum, u32 base, u32 lo, u32 hi, u32 r) {
    while (lo < hi) { const u32 mid = lo + (hi - lo + 1u) / 2u; if (cum[mid] - base <= r) lo = mid; else hi = mid - 1u; }
    return lo;
}
// the reads of a stretch that stay, added to their entries
__global__ __launch_bounds__(TPB) void k_ds_count(const u32* stretch0, u32 n_large, const DsState* state, const int* indptr_n, const u32* cum, u64 seed,
                                                  int* out) {
    __shared__ u32 s_l;
    u32 r0;
    const u32 l = ds_stretch_sample(stretch0, n_large, &s_l, &r0);
    const DsState st = state[l];
    const u32 a = (u32)indptr_n[st.sample], last = (u32)indptr_n[st.sample + 1] - 1u, base = cum[a], nd = st.depth + 1u;
    r0 += threadIdx.x * DS_THREAD_READS;
    const bool valid = r0 < st.reads;
    u32 j = a, acc = 0;
    if (valid) {
        j = ds_entry_of(cum, base, a, last, r0);
        u32 end = cum[j + 1] - base;                 // the first read beyond entry j
#pragma unroll 4
        for (u32 i = 0; i < DS_THREAD_READS; ++i) {
            const u32 r = r0 + i;
            if (r >= st.reads) break;
            if (r >= end) {
                if (acc) atomicAdd(out + j, (int)acc);
                acc = 0;
                j = ds_entry_of(cum, base, j + 1u, last, r);
                end = cum[j + 1] - base;
            }
            acc += ds_at_most(ds_key(seed, st.sample, r), st.pfx, nd);
        }
    }
    // a wave whose threads all ended in one entry (an entry of a million reads is a thousand such waves) sends one add
    const u64 have = __ballot(valid);
    if (!have) return;
    const u32 fj = (u32)__shfl((int)j, __ffsll((long long)have) - 1);
    if (__ballot(valid && j == fj) == have) {
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) acc += __shfl_xor(acc, w);
        if ((threadIdx.x & 63u) == 0u && acc) atomicAdd(out + fj, (int)acc);
    } else if (acc) atomicAdd(out + j, (int)acc);
}

int ds_check_args(uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* indptr_n, const void* indices_n, const void* data_n, const void* target,
                  const void* out_data_n, const void* in_total, const void* out_total) {
    if (!indptr_n || !target || (nnz_n && (!indices_n || !data_n || !out_data_n)))
        return fail(nullptr, ECB_ERR_ARG, "downsample: bad argument (no N, no target or no out_data_n)");
    if (n_ecs >= (1u << 31) - 1u || nnz_n >= (1ull << 31) || n_samples >= (1u << 31) - 1u)
        return fail(nullptr, ECB_ERR_LIMIT, "the matrices exceed the .bin format's int32 limits");
    const u64 S = n_samples, zn = nnz_n * 4;
    const uintptr_t words32 = (uintptr_t)indptr_n | (uintptr_t)indices_n | (uintptr_t)data_n | (uintptr_t)out_data_n;
    const uintptr_t words64 = (uintptr_t)target | (uintptr_t)in_total | (uintptr_t)out_total;
    if ((words32 & 3u) || (words64 & 7u)) return fail(nullptr, ECB_ERR_ARG, "downsample: a pointer that is not aligned to its element");
    if (span_clash({{indptr_n, (S + 1) * 4}, {indices_n, zn}, {data_n, zn}, {target, S * 8}, {out_data_n, zn}, {in_total, in_total ? S * 8 : 0},
                    {out_total, out_total ? S * 8 : 0}}, 3))
        return fail(nullptr, ECB_ERR_ARG, "downsample: an output overlaps an input or another output");
    return ECB_OK;
}
}  // namespace

extern "C" int ecb_downsample_device(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const void* d_indptr_n, const void* d_indices_n,
                                     const void* d_data_n, const void* d_target, uint64_t seed, void* d_out_data_n, void* d_in_total, void* d_out_total) {
    RCCHK(ds_check_args(n_ecs, n_samples, nnz_n, d_indptr_n, d_indices_n, d_data_n, d_target, d_out_data_n, d_in_total, d_out_total));
    Call c(device, "downsample: "); if (c.rc) return c.rc;
    hipStream_t st = c.st;
    const u64 S = n_samples;
    const int *pn = (const int*)d_indptr_n, *xn = (const int*)d_indices_n, *dn = (const int*)d_data_n;
    const long long* target = (const long long*)d_target;
    int* out = (int*)d_out_data_n;
    u64* words;
    RCCHK(c.status_words(words, DS_WORDS, 0));
    // what is sized by N alone is cut from one pool buffer: two 8-byte and five 4-byte arrays per sample, the prefix sums of the counts, one
    // scan's scratch; what is sized by the number of large samples comes from two more once that is known
    Arena ar(c, CV_X0, 2 * Arena::pad(S, 8) + 5 * Arena::pad(S + 1, 4) + Arena::pad(nnz_n + 1, 4) + Arena::pad(scan_words(std::max<u64>(S, nnz_n) + 1), 4));
    u64* tot = ar.take<u64>(S);
    long long* otot = ar.take<long long>(S);
    u32 *mode = ar.take<u32>(S), *large = ar.take<u32>(S), *stretches = ar.take<u32>(S), *lpos = ar.take<u32>(S + 1), *spos = ar.take<u32>(S + 1);
    u32 *cum = ar.take<u32>(nnz_n + 1), *sums = ar.take<u32>(scan_words(std::max<u64>(S, nnz_n) + 1));
    RCCHK(ar.missing(c));
    // 1. N checked, the totals, a mode per sample (nothing here follows an index that has not been checked: a malformed N gives totals
    // that nobody reads)
    CALLCHK(c, hipMemsetAsync(tot, 0, std::max<u64>(S, 1) * 8, st));
    k_sel_ncheck<<<nblk(std::max<u64>(nnz_n, S + 1), TPB), TPB, 0, st>>>(pn, n_samples, xn, dn, nnz_n, n_ecs, words);
    if (S && nnz_n) k_sel_totals<<<nblk(nnz_n, SEL_TPB * SEL_ITEMS), SEL_TPB, 0, st>>>(pn, n_samples, xn, dn, nnz_n, nullptr, tot);
    if (S) {
        k_ds_plan<<<nblk(S, TPB), TPB, 0, st>>>(tot, target, n_samples, mode, otot, large, stretches, words);
        CALLCHK(c, hipGetLastError());
        CALLCHK(c, scan_launch(st, large, S, lpos, sums, words + DS_W_LARGE));
        CALLCHK(c, scan_launch(st, stretches, S, spos, sums, words + DS_W_STRETCHES));
    }
    CALLCHK(c, hipGetLastError());
    u64 back[DS_WORDS];
    RCCHK(c.read_back(back, words, DS_WORDS));
    RCCHK(refuse_bits(nullptr, CA_ERRS, (u32)back[DS_W_ERR]));
    if (back[DS_W_LIMIT]) return fail(nullptr, ECB_ERR_LIMIT, "downsample: a sample to thin holds 2^31 reads or more");
    if (back[DS_W_STRETCHES] >= DS_MAX_STRETCHES) return fail(nullptr, ECB_ERR_LIMIT, "downsample: the samples to thin hold 2^31 stretches of %u reads or more", DS_WG_READS);
    // the input is well formed: from here on the outputs are written
    const u64 n_small = back[DS_W_SMALL], n_large = back[DS_W_LARGE], n_stretches = back[DS_W_STRETCHES];
    if (S && d_in_total) CALLCHK(c, hipMemcpyAsync(d_in_total, tot, S * 8, hipMemcpyDeviceToDevice, st));
    if (S && d_out_total) CALLCHK(c, hipMemcpyAsync(d_out_total, otot, S * 8, hipMemcpyDeviceToDevice, st));
    if (nnz_n && !back[DS_W_CHANGED]) CALLCHK(c, hipMemcpyAsync(out, dn, nnz_n * 4, hipMemcpyDeviceToDevice, st));      // no sample thinned or emptied: a copy
    else if (nnz_n) {
        // 2. the columns that are copied or emptied
        k_ds_init<<<nblk(nnz_n, SEL_TPB * SEL_ITEMS), SEL_TPB, 0, st>>>(pn, n_samples, dn, nnz_n, mode, out);
        // 3. the small samples
        if (n_small) k_ds_small<<<n_samples, TPB, 0, st>>>(pn, dn, mode, target, seed, out);
        CALLCHK(c, hipGetLastError());
    }
    // 4. the large samples
    if (n_large) {
        DsState* state = c.get<DsState>(CV_X1, n_large);
        u32 *stretch0 = c.get<u32>(CV_X2, n_large + 1), *hist = c.get<u32>(CV_X3, n_large * DS_BINS);
        RCCHK(c.missing());
        CALLCHK(c, hipMemsetAsync(hist, 0, n_large * DS_BINS * 4, st));
        CALLCHK(c, scan_launch(st, (const u32*)dn, nnz_n, cum, sums, nullptr, 1, cum + nnz_n));
        k_ds_large_init<<<nblk(S, TPB), TPB, 0, st>>>(mode, lpos, spos, tot, target, n_samples, (u32)n_large, (u32)n_stretches, state, stretch0);
        CALLCHK(c, hipGetLastError());
        u64 open = n_large;
        for (u32 d = 0; d < DS_DIGITS && open; ++d) {
            CALLCHK(c, hipMemsetAsync(words + DS_W_OPEN, 0, 8, st));
            k_ds_hist<<<(unsigned)n_stretches, TPB, 0, st>>>(stretch0, (u32)n_large, state, seed, d, hist);
            k_ds_pick<<<(unsigned)n_large, TPB, 0, st>>>(state, hist, d, words);
            CALLCHK(c, hipGetLastError());
            RCCHK(c.read_back(&open, words + DS_W_OPEN, 1));
        }
        if (open) return fail(nullptr, ECB_ERR_HIP, "downsample: a sample unresolved after the last digit (internal)");
        k_ds_count<<<(unsigned)n_stretches, TPB, 0, st>>>(stretch0, (u32)n_large, state, pn, cum, seed, out);
        CALLCHK(c, hipGetLastError());
    }
    CALLCHK(c, hipStreamSynchronize(st));
    return ECB_OK;
}

extern "C" int ecb_downsample(int device, uint32_t n_ecs, uint32_t n_samples, uint64_t nnz_n, const int32_t* indptr_n, const int32_t* indices_n,
                              const int32_t* data_n, const int64_t* target, uint64_t seed, int32_t* out_data_n, int64_t* in_total, int64_t* out_total) {
    RCCHK(ds_check_args(n_ecs, n_samples, nnz_n, indptr_n, indices_n, data_n, target, out_data_n, in_total, out_total));
    Call c(device, "downsample: "); if (c.rc) return c.rc;
    const u64 S = n_samples;
    DevBuf<> ipn, ixn, dan, tg, od, it, ot;
    RCCHK(stage_in(c, {{&ipn, indptr_n, (S + 1) * 4}, {&ixn, indices_n, nnz_n * 4}, {&dan, data_n, nnz_n * 4}, {&tg, target, S * 8}, {&od, nullptr, nnz_n * 4},
                       {&it, nullptr, S * 8}, {&ot, nullptr, S * 8}}));
    RCCHK(ecb_downsample_device(device, n_ecs, n_samples, nnz_n, ipn.p, ixn.p, dan.p, tg.p, seed, od.p, in_total ? it.p : nullptr, out_total ? ot.p : nullptr));
    return stage_out(c, {{out_data_n, &od, nnz_n * 4}, {in_total, &it, in_total ? S * 8 : 0}, {out_total, &ot, out_total ? S * 8 : 0}});
}
