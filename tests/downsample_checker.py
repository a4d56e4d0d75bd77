"""ecdownsample's yardstick, in numpy and Python integers: ``include/ecb_downsample.h`` restated -- the 128-bit key of a read from
``boot_checker``'s Philox, the ``n`` smallest keys by ``np.lexsort``, the count per entry by ``searchsorted`` -- and the file command
restated on top of it and ``select_checker``.  Nothing here is taken from the library."""
import copy

import numpy as np

import boot_checker as bc
import select_checker

MAX_READS = 1 << 31


def key_words(seed, s, r):
    """(o0, o1, o2, o3) of reads ``r`` (an int or an array) of sample ``s``: Philox4x32-10 at counter (r, 0, s, 1) under the seed's halves."""
    r = np.asarray(r, dtype=np.uint64)
    z = np.zeros_like(r)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return bc.philox((r, z, z + np.uint64(s), z + np.uint64(1)), (seed & bc.MASK, seed >> 32))


def key(seed, s, r):
    """The key of one read as a Python integer below 2^128."""
    o = [int(v) for v in key_words(seed, s, r)]
    return o[3] << 96 | o[2] << 64 | o[1] << 32 | o[0]


def digit(k, d):
    """8-bit digit d of a key: 0 = the most significant, 15 = the least."""
    return (k >> (8 * (15 - d))) & 255


def kept_reads(seed, s, M, n):
    """The numbers of the ``n`` reads of sample ``s`` (of ``M`` reads, 0 < n < M) that stay, ascending."""
    o0, o1, o2, o3 = key_words(seed, s, np.arange(M))
    order = np.lexsort((o0, o1, o2, o3))                        # (the last key is the primary one)
    return np.sort(order[:n])


def thin_column(counts, s, n, seed):
    """One column's counts after the draw: int64, one per entry."""
    counts = np.asarray(counts, dtype=np.int64)
    M = int(counts.sum())
    if n < 0 or n >= M:
        return counts.copy()
    if n == 0:
        return np.zeros_like(counts)
    if M >= MAX_READS:
        raise OverflowError("a sample to thin holds 2^31 reads or more")
    cum = np.cumsum(counts)
    entry = np.searchsorted(cum, kept_reads(seed, s, M, n), side="right")      # read r is of the entry j with cum[j - 1] <= r < cum[j]
    return np.bincount(entry, minlength=len(counts)).astype(np.int64)


def breach(indptr_n, indices_n, data_n, n_ecs):
    """None, or what is wrong with N, as the library's three refusals word it."""
    ptr, ec, cnt = (np.asarray(a, dtype=np.int64) for a in (indptr_n, indices_n, data_n))
    if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(ec) or (np.diff(ptr) < 0).any() or (ptr < 0).any() or (ptr > len(ec)).any():
        return "column pointers"
    if ((ec < 0) | (ec >= n_ecs)).any():
        return "an EC index at or beyond n_ecs"
    if (cnt < 0).any():
        return "a negative count"
    return None


def downsample(indptr_n, indices_n, data_n, n_ecs, target, seed=0):
    """``ecb_downsample`` -> (out_data_n int32, in_total int64, out_total int64)."""
    assert breach(indptr_n, indices_n, data_n, n_ecs) is None
    ptr, cnt = np.asarray(indptr_n, dtype=np.int64), np.asarray(data_n, dtype=np.int64)
    S = len(ptr) - 1
    out = np.zeros(len(cnt), dtype=np.int64)
    tin, tout = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    for s in range(S):
        a, b = int(ptr[s]), int(ptr[s + 1])
        out[a:b] = thin_column(cnt[a:b], s, int(target[s]), seed)
        tin[s], tout[s] = cnt[a:b].sum(), out[a:b].sum()
    return out.astype(np.int32), tin, tout


def brute_column(counts, s, n, seed):
    """The same by a sort of Python tuples (key, read, entry): what the checker itself is held to."""
    reads = [(key(seed, s, r), r, j) for j, r in zip(np.repeat(np.arange(len(counts)), counts), range(int(np.sum(counts))))]
    M = len(reads)
    if n < 0 or n >= M:
        return [int(c) for c in counts]
    out = [0] * len(counts)
    for _, _, j in sorted(reads)[:n]:
        out[j] += 1
    return out


# ---- the file command -----------------------------------------------------------------------------------------------------------------------
def totals(m):
    ptr = m.indptrN.astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(m.dataN.astype(np.int64))])
    return cum[ptr[1:]] - cum[ptr[:-1]]


def staying(m, samples=None, mincount=None):
    """Step 2: the named samples (None: all) with at least max(mincount, 1) reads."""
    return select_checker.named(m, samples) & (totals(m) >= max(int(mincount or 0), 1))


def targets(m, stay, reads=None, fraction=None, equalize=False):
    """Step 3: the target per column of the input, -1 for the samples that do not stay."""
    M = totals(m)
    t = np.full(m.num_samples, -1, dtype=np.int64)
    for s in np.flatnonzero(stay):
        if reads is not None:
            t[s] = int(reads)
        elif fraction is not None:
            t[s] = int(np.floor(np.float64(fraction) * np.float64(M[s])))
        else:
            t[s] = int(M[stay].min())
    return t


def ecdownsample(m, reads=None, fraction=None, equalize=False, seed=0, samples=None, mincount=None):
    """The command on an ``ECMatrices`` -> (the result, the stats rows ``(sample, reads_in, reads_out, ecs_in, ecs_out)``)."""
    stay = staying(m, samples, mincount)
    t = targets(m, stay, reads, fraction, equalize)
    thin, tin, tout = downsample(m.indptrN, m.indicesN, m.dataN, m.num_reads, t, seed)
    ptr = m.indptrN.astype(np.int64)
    nz = lambda d: [int((np.asarray(d[ptr[s]:ptr[s + 1]]) > 0).sum()) for s in range(m.num_samples)]      # noqa: E731
    ein, eout = nz(m.dataN), nz(thin)
    stats = [(m.sname[s], int(tin[s]), int(tout[s]), ein[s], eout[s]) for s in np.flatnonzero(stay)]
    thinned = copy.copy(m)
    thinned.dataN = thin
    return select_checker.select_flags(thinned, None, stay, 1)[0], stats


def ecdownsample_bytes(m, **kw):
    from alntools_amd import bin_utils
    return bin_utils.ecsave2_bytes(ecdownsample(m, **kw)[0])
