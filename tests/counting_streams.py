"""Read streams for ``test_gpu_counting.py``, what they must give, and the arithmetic by which the counting pass behind ``k_stream``
(``ensure_counts``, ``alntools_amd/csrc/ecb.hip``) picks its path -- all known without a device.

Read ``r`` carries the records of EC template ``tpl[r]``; read ids run 0, 1, 2 ... in order.  Template ``k`` is ``1 + k % 3`` records
on loci ``3k, 3k + 1, 3k + 2`` (``one_record``: one record on locus ``k``), record ``w`` on haplotype ``(k + w) % H`` -- templates
share no locus, so they are distinct ECs.  The expected result then follows from ``tpl`` alone, in 64-bit numpy: ECs in order of
first appearance, ``N`` = reads per EC, the EC id of every read, CSR ``A`` = the templates' records in that order
(``bam_utils.py:309-312, 688-698`` of the reference).  ``test_counting_streams.py`` holds this shortcut against the C oracle, which is
pinned to the reference's goldens, on every named stream small enough for both."""
import numpy as np

H = 4
ORACLE_MAX_READS = 1100000        # streams up to here are also compared with the C oracle (on the CPU and on the GPU)


class Stream(object):
    def __init__(self, tpl, one_record=False, n_loci=None):
        self.tpl = np.ascontiguousarray(tpl, dtype=np.int64)
        assert self.tpl.ndim == 1 and len(self.tpl) and self.tpl.min() >= 0
        self.one_record = one_record
        self.stride = 1 if one_record else 3
        self.n_reads = len(self.tpl)
        self.n_loci = n_loci or self.stride * (int(self.tpl.max()) + 1)
        assert self.n_loci >= self.stride * (int(self.tpl.max()) + 1)

    def _n_rec(self, t):
        return np.ones(len(t), np.int64) if self.one_record else 1 + t % 3

    def _records(self, t):
        """Records of the templates ``t``, row after row -> (row of every record, locus, haplotype)."""
        n_rec = self._n_rec(t)
        row = np.repeat(np.arange(len(t), dtype=np.int64), n_rec)
        w = np.arange(len(row), dtype=np.int64) - np.repeat(np.cumsum(n_rec) - n_rec, n_rec)
        tt = t[row]
        return row, self.stride * tt + w, (tt + w) % H

    def tuples(self):
        """-> (read_id, locus, hapflag) as libecb takes them (uint32; the haplotype sits above bit 16, no filter flag is set)."""
        row, locus, hap = self._records(self.tpl)
        return row.astype(np.uint32), locus.astype(np.uint32), (hap << 16).astype(np.uint32)

    def shard(self, r0, r1):
        """Reads [r0, r1) as a stream of their own (read ids from 0), over the same loci."""
        return Stream(self.tpl[r0:r1], self.one_record, self.n_loci)

    def expected(self):
        """-> dict(indptr, indices, data, count, first, read_ec, sizes): int64 arrays (``first`` = every EC's first read), ``sizes``
        as ``ecb_finalize`` reports them."""
        uniq, first = np.unique(self.tpl, return_index=True)
        order = np.argsort(first, kind="stable")
        t = uniq[order]                                                  # templates in order of first appearance
        rank_of = np.full(int(uniq[-1]) + 1, -1, np.int64)
        rank_of[t] = np.arange(len(t))
        read_ec = rank_of[self.tpl]
        count = np.bincount(self.tpl, minlength=len(rank_of))[t]          # N = bincount(tpl), re-ordered by first occurrence
        row, locus, hap = self._records(t)
        indptr = np.concatenate(([0], np.cumsum(self._n_rec(t))))
        n_rec = int(self._n_rec(self.tpl).sum())
        sizes = dict(n_ecs=len(t), nnz_a=int(indptr[-1]), n_samples=1, nnz_n=len(t), all_alignments=n_rec, valid_alignments=n_rec,
                     n_reads=self.n_reads)
        return dict(indptr=indptr, indices=locus, data=np.int64(1) << hap, count=count, first=first[order], read_ec=read_ec,
                    sizes=sizes)


def concat(a, b):
    """Stream ``a`` followed by stream ``b``."""
    assert a.one_record == b.one_record
    return Stream(np.concatenate((a.tpl, b.tpl)), a.one_record, max(a.n_loci, b.n_loci))


# ---- the pass's arithmetic, restated (constants pinned by test_threshold_constants.py) -------------------------------------------
BIN_BITS, MIN_BIN_BITS, MAX_BIN_BITS, MAX_BUCKETS = 14, 11, 15, 8192
PART_G, PART_READS, STAGE, STAGE_MAX_BUCKETS = 512, 4096, 8192, 4096
PIECE_MIN = 32768
BM_LINE_READS = 16 * 32          # reads per bitmap line (BM_LINE words)
SCB = 1024 * 16                  # values per stretch of the look-back scan (SCB_TPB * SCB_ITEMS)


def table_slots(ec_capacity):
    """``ecb_create``: the next power of two, at least 1024."""
    return max(1 << (ec_capacity - 1).bit_length(), 1024)


def ranges(cap, bin_bits=None):
    """``ensure_counts`` -> (bb, nb): slots per range 2^bb, number of ranges; ``bin_bits`` = the ECB_BIN_BITS knob."""
    lc = cap.bit_length() - 1
    bb = min(max(lc, 9 + MIN_BIN_BITS) - 9, BIN_BITS)
    if bin_bits is not None:
        bb = min(max(bin_bits, MIN_BIN_BITS), MAX_BIN_BITS)
    while bb < MAX_BIN_BITS and (cap >> bb) > MAX_BUCKETS:
        bb += 1
    return bb, max(1, cap >> bb)


def piece(n_reads, nb):
    return max(PIECE_MIN, 2 * -(-n_reads // nb))


def pieces(length, pc):
    """``k_build_work``: work items of a range of ``length`` reads (1 = whole: the only writer of its slots)."""
    return -(-length // pc) if length > pc + pc // 2 else (1 if length else 0)


def partition(n_reads):
    """-> (G, part_per, reads of every workgroup of the partition passes)."""
    g = min(PART_G, -(-n_reads // PART_READS))
    per = (-(-n_reads // g) + 3) & ~3
    return g, per, [max(0, min(per, n_reads - i * per)) for i in range(g)]


def bitmap_lines(n_reads):
    return ((n_reads + 31) // 32 + 16) // 16


# ---- template choice per read, seeded --------------------------------------------------------------------------------------------
def uniform(n_reads, n_tpl, seed):
    return np.random.default_rng(seed).integers(0, n_tpl, n_reads)


def each_once(n_reads, seed):
    """Every EC once: every count is 1, the list of occupied slots is as long as the stream."""
    return np.random.default_rng(seed).permutation(n_reads)


def degenerate(counts, seed):
    """Every read in one of ``len(counts)`` templates, template ``i`` exactly ``counts[i]`` times, in random order."""
    tpl = np.repeat(np.arange(len(counts)), counts)
    return np.random.default_rng(seed).permutation(tpl)


def hot_interleaved(n_reads, n_tpl, k, seed):
    """Every other read in one of ``k`` hot templates (ids ``n_tpl .. n_tpl + k - 1``, taken in turn), the rest uniform over
    ``n_tpl``: a wave of the counting kernel sees a hot slot in about half its lanes."""
    tpl = uniform(n_reads, n_tpl, seed)
    tpl[::2] = n_tpl + (np.arange(len(tpl[::2])) % k)
    return tpl


def hot_bunched(n_reads, n_tpl, k, share, run, seed):
    """``k`` hot templates (ids from ``n_tpl``) hold ``share`` of the reads in runs of ``run`` reads of one template (whole waves
    see one slot), at random places between reads uniform over ``n_tpl``."""
    rng = np.random.default_rng(seed)
    n_runs = int(n_reads * share) // run
    n_cold = n_reads - n_runs * run
    cuts = np.sort(rng.integers(0, n_cold + 1, n_runs))
    cold = rng.integers(0, n_tpl, n_cold)
    parts, at = [], 0
    for i, c in enumerate(cuts.tolist()):
        parts += [cold[at:c], np.full(run, n_tpl + i % k)]
        at = c
    parts.append(cold[at:])
    return np.concatenate(parts)


def runs_between_uniform(lengths, n_tpl, seed, reps=3):
    """Runs of one template of every length in ``lengths``, each at once followed by a run of the same length of a second hot
    template (two hot slots in one wave), between 20 .. 120 reads uniform over ``n_tpl``.  The run of length ``lengths[i]`` is of
    template ``n_tpl + 1 + i``; the second hot template is ``n_tpl``."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(reps):
        for i, n in enumerate(lengths):
            parts += [rng.integers(0, n_tpl, int(rng.integers(20, 121))), np.full(n, n_tpl + 1 + i), np.full(n, n_tpl)]
    parts.append(rng.integers(0, n_tpl, 77))
    return np.concatenate(parts)


def firsts_at(n_reads, positions, n_base, seed=None):
    """ECs whose first reads are the reads ``positions`` (each a template of its own, seen only there), every other read a repeat
    of one of ``n_base`` templates that all appear in the first ``n_base`` reads."""
    positions = np.asarray(sorted(positions), np.int64)
    assert positions[0] >= n_base and positions[-1] < n_reads and len(np.unique(positions)) == len(positions)
    if seed is None:
        tpl = np.arange(n_reads, dtype=np.int64) % n_base
    else:
        tpl = np.random.default_rng(seed).integers(0, n_base, n_reads)
        tpl[:n_base] = np.arange(n_base)
    tpl[positions] = n_base + np.arange(len(positions))
    return tpl


# ---- the named streams (every one of them is held against the C oracle on the CPU if it is small enough) -------------------------
R1 = 1000003                       # "about a million reads", odd: the 16-byte loads of every pass have a ragged end
G1_TEMPLATES = (200, 1 << 13, 1 << 19)
EDGE_READS = (1, 2, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, 2097151, 2097152, 2097153)
RUN_LENGTHS = tuple(range(1, 10)) + (63, 64, 65, 8 * 1024 - 1, 8 * 1024, 8 * 1024 + 1)
LINE_FIRSTS = (510, 511, 512, 513, 16383, 16384)
BIG_READS = 8388608 + 4096        # the scan over the bitmap lines' popcounts starts its second stretch at read 8 388 608

STREAMS = {}


def _named(name, make):
    assert name not in STREAMS
    STREAMS[name] = make


for _e in G1_TEMPLATES:
    _named("g1_uniform_%d" % _e, lambda e=_e: Stream(uniform(R1, e, 11)))
    _named("g1_hot1_interleaved_%d" % _e, lambda e=_e: Stream(hot_interleaved(R1, e, 1, 12)))
    _named("g1_hot3_bunched_%d" % _e, lambda e=_e: Stream(hot_bunched(R1, e, 3, 0.6, 3000, 13)))
_named("g1_each_once", lambda: Stream(each_once((1 << 19) + 1, 14)))
for _i, _r in enumerate(EDGE_READS):                # degenerate: every read in one of 1, 2 or 5 templates, in turn over the read counts
    _named("g2_uniform_%d" % _r, lambda r=_r: Stream(uniform(r, 100, 20 + r % 7)))
    _named("g2_degenerate_%d" % _r, lambda r=_r, k=(1, 2, 5)[_i % 3]: Stream(uniform(r, k, 30 + r % 7)))
# cut ranges: piece = 32768 at these sizes, a range is cut from 49 153 reads on
_named("g3_one_ec_49152", lambda: Stream(degenerate([49152], 40)))
_named("g3_one_ec_49153", lambda: Stream(degenerate([49153], 41)))
_named("g3_one_ec_many_pieces", lambda: Stream(degenerate([1000001], 42)))
_named("g3_two_ecs_on_the_limit", lambda: Stream(degenerate([49152, 49153], 43)))
_named("g3_five_ecs", lambda: Stream(degenerate([200001, 49153, 65537, 300000, 98305], 44)))
_named("g3_hot_bunched_in_uniform", lambda: Stream(hot_bunched(400001, 200, 1, 0.3, 4000, 45)))
_named("g3_hot_interleaved_in_uniform", lambda: Stream(hot_interleaved(300001, 200, 1, 46)))
_named("g4_runs", lambda: Stream(runs_between_uniform(RUN_LENGTHS, 60, 50)))
_named("g5_line_firsts", lambda: Stream(firsts_at(20000, LINE_FIRSTS + (19999,), 7)))
_named("g6_own", lambda: Stream(hot_bunched(150001, 150, 1, 0.5, 2500, 60), n_loci=3 * 260))
_named("g6_other", lambda: Stream(np.concatenate((uniform(90001, 150, 61) + 100, np.full(60000, 150))), n_loci=3 * 260))


def big_ranking_stream():
    """8 388 608 + 4096 one-record reads; first appearances at reads 8 388 607 and 8 388 608, 3000 more before them, 1000 more
    behind, and at the last read.  (Not in STREAMS: numpy alone says what it gives.)"""
    rng = np.random.default_rng(70)
    edge = 8388608
    pos = np.concatenate((rng.choice(np.arange(50, edge - 1), 3000, replace=False), [edge - 1, edge],
                          rng.choice(np.arange(edge + 1, BIG_READS - 1), 1000, replace=False), [BIG_READS - 1]))
    return Stream(firsts_at(BIG_READS, pos, 50, seed=71), one_record=True)
