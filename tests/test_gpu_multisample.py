"""The multisample back end (``ms_reduce`` -> ``ecb_ms_filter``, ``bam2ec --multisample``) on every path it takes, against what the
stream was built to hold.

Every read here carries the records of one EC template, so the expected (EC, cell, file) triples follow from how the stream is made,
not from the device: an EC's rank is the order in which its template first appears, a triple's count is its reads, its first read the
smallest of them.  Those expected triples go through ``ms_checker`` (the numpy restatement of bam_utils_multisample.py:503-636,
737-791) for the expected filter result.  Reads sit in their files in contiguous ranges, files in order, as a directory scan gives them.

Constants of ``ecb.hip`` the inputs straddle (pinned by ``test_threshold_constants.py``): MSF_LDS_CELLS = 8192 (per-cell counters in
LDS up to it, global atomics above), MSF_SMALL = 256 (triples of an EC taken by one thread up to it, by one workgroup above),
MSF_GIANT = 32768 (above it an EC is shared over the whole grid), RS_TILE = 4096 (the radix sort's tile: the cell order sorts the cells
that have reads); and the meta word: cell ids below 2^22 (ECB_CELL_BITS), files up to 1023."""
import numpy as np
import pytest

from alntools_amd import ecb
from ms_checker import reduce_triples, select_rows

pytestmark = pytest.mark.gpu

H = 4
CELL_BITS = 22
MAX_CELLS = 1 << CELL_BITS
LDS_CELLS, SMALL, GIANT = 8192, 256, 32768
I32 = (1 << 31) - 1


# ---- streams ---------------------------------------------------------------------------------------------------------------------
class Stream(object):
    """Reads in order, one EC template each: template k = {locus 2k: haplotype k % H} and, for k % 3 == 0, also {locus 2k + 1:
    haplotype (k + 1) % H} -- distinct sets, so distinct ECs."""

    def __init__(self, tpl, cell, fil):
        self.tpl, self.cell, self.file = (np.asarray(a, np.int64) for a in (tpl, cell, fil))
        assert self.cell.max() < MAX_CELLS and self.file.max() < 1024
        self.n_reads = len(self.tpl)
        self.n_loci = 2 * int(self.tpl.max()) + 2
        n_rec = 1 + (self.tpl % 3 == 0)
        idx = np.repeat(np.arange(self.n_reads), n_rec)
        w = np.arange(len(idx)) - np.repeat(np.cumsum(n_rec) - n_rec, n_rec)
        t = self.tpl[idx]
        self.read_id, self.locus = idx.astype(np.uint32), (2 * t + w).astype(np.uint32)
        self.hapflag = ((((t + w) % H) << 16)).astype(np.uint32)
        self.meta = (self.cell | (self.file << CELL_BITS)).astype(np.uint32)

    def records(self, r0, r1):
        """Tuples of reads [r0, r1), read ids from 0."""
        a, b = np.searchsorted(self.read_id, [r0, r1])
        return self.read_id[a:b] - np.uint32(r0), self.locus[a:b], self.hapflag[a:b]

    def ec_of_read(self):
        """-> (EC rank of every read, template of every EC in rank order): ranks in order of first appearance."""
        uniq, first_idx, inv = np.unique(self.tpl, return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), np.int64)
        rank[np.argsort(first_idx)] = np.arange(len(uniq))
        return rank[inv.ravel()], uniq[np.argsort(rank)]

    def expected(self):
        """-> (triples dict sorted by (EC, cell, file), number of ECs, CSR A in rank order)."""
        ec, t = self.ec_of_read()
        key = (ec << 32) | (self.cell << 10) | self.file
        order = np.argsort(key, kind="stable")
        ks = key[order]
        heads = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
        k = ks[heads]
        tr = dict(ec=k >> 32, cell=(k >> 10) & (MAX_CELLS - 1), file=k & 1023, count=np.diff(np.concatenate((heads, [len(ks)]))),
                  first=order[heads])                                 # (stable: the first of a run is its smallest read)
        two = t % 3 == 0
        indptr = np.concatenate(([0], np.cumsum(1 + two)))
        indices = np.empty(indptr[-1], np.int64)
        data = np.empty(indptr[-1], np.int64)
        indices[indptr[:-1]], data[indptr[:-1]] = 2 * t, 1 << (t % H)
        indices[indptr[1:][two] - 1], data[indptr[1:][two] - 1] = 2 * t[two] + 1, 1 << ((t[two] + 1) % H)
        return tr, len(t), (indptr, indices, data)


def _in_file_order(rng, tpl, cell, fil):
    """Reads sorted by file, in random order within a file."""
    o = np.lexsort((rng.random(len(fil)), fil))
    return Stream(np.asarray(tpl)[o], np.asarray(cell)[o], np.asarray(fil)[o])


def _random_stream(rng, cells, n_reads, n_files, n_tpl=4000, pinned=()):
    """Every cell of ``cells`` has reads; the rest of the reads go to cells and files at random, templates Zipf-distributed (a few ECs
    of tens of thousands of triples, many of a handful).  ``pinned``: (cell, file) of reads added on top."""
    cells = np.asarray(cells, np.int64)
    pc, pf = (np.asarray([p[i] for p in pinned], np.int64) for i in (0, 1))
    cell = np.concatenate((cells, cells[rng.integers(0, len(cells), n_reads - len(cells))], pc))
    fil = np.concatenate((rng.integers(0, n_files, n_reads), pf))
    tpl = (rng.zipf(1.5, len(cell)) - 1) % n_tpl
    return _in_file_order(rng, tpl, cell, fil)


# ---- running and checking --------------------------------------------------------------------------------------------------------
def _builder(st, device=False):
    b = ecb.EcBuilder(st.n_loci, H, multisample=True)
    _push(b, st, device)
    return b


def _push(b, st, device=False):
    if device:
        import torch
        d = [torch.from_numpy(a.view(np.int32)).cuda() for a in (st.read_id, st.locus, st.hapflag, st.meta)]
        torch.cuda.synchronize()
        b.push_device(d[0], d[1], d[2])
        b.push_cells_device(d[3], 0)
        b._keep = d                                                   # (alive until finalize)
    else:
        b.push(st.read_id, st.locus, st.hapflag)
        b.push_cells(st.meta, 0)


def _check_built(b, st, exp):
    """finalize / export / export_pairs of a handle that holds ``st`` == what ``st`` was built to hold."""
    tr, n_ecs, (ip, ix, da) = exp
    s = b.finalize()
    assert s["n_reads"] == st.n_reads and s["n_ecs"] == n_ecs and s["nnz_n"] == len(tr["ec"])
    a = b.export()
    assert np.array_equal(a["indptrA"], ip) and np.array_equal(a["indicesA"], ix) and np.array_equal(a["dataA"], da)
    got = b.export_pairs()
    for k in ("ec", "cell", "file", "count", "first"):
        assert np.array_equal(got[k], tr[k]), k
    assert int(got["count"].sum()) == st.n_reads
    return a


def _check_filter(b, a, tr, n_ecs, n_cells, mincount):
    """ms_filter(n_cells, mincount) == the checker on the expected triples; a filter that keeps no cell must refuse (-7)."""
    kept, ec_keep, (n_ptr, n_idx, n_dat) = reduce_triples(tr, n_ecs, n_cells, mincount)
    if not kept:
        with pytest.raises(ecb.EcbError) as e:
            b.ms_filter(n_cells, mincount)
        assert e.value.code == -7
        return kept
    f = b.ms_filter(n_cells, mincount)
    assert f["kept_cells"].tolist() == kept, mincount
    assert f["n_cells_seen"] == len(np.unique(tr["cell"]))
    a_ptr, a_idx, a_dat = select_rows(a["indptrA"], a["indicesA"], a["dataA"], ec_keep)
    for k, e in (("indptrA", a_ptr), ("indicesA", a_idx), ("dataA", a_dat), ("indptrN", n_ptr), ("indicesN", n_idx), ("dataN", n_dat)):
        assert np.array_equal(f[k], e), (k, mincount)
    totals = np.bincount(tr["cell"], weights=tr["count"], minlength=n_cells).astype(np.int64)
    assert int(f["dataN"].astype(np.int64).sum()) == int(totals[kept].sum())        # the kept cells' reads, every one
    return kept


def _triples_per_ec(tr, n_ecs):
    return np.bincount(tr["ec"], minlength=n_ecs)


# ---- cell counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells,seen,device", [
    (4096, 4095, False),                 # LDS path; the cell order sorts one cell less than a radix tile
    (4097, 4096, False),                 # LDS path; a tile of cells
    (8192, 4097, False),                 # the last LDS size; a tile and one
    (8193, 8192, True),                  # the first global size; pushed from device memory
    (300_000, 100_000, False),           # a run's worth of barcodes
    (MAX_CELLS, 150_000, False),         # every cell id the meta word has
], ids=["4096", "4097", "8192", "8193", "300000", "2^22"])
def test_cell_counts_on_the_lds_limit_and_the_radix_tile(n_cells, seen, device):
    """n_cells on both sides of MSF_LDS_CELLS, cells with reads on both sides of RS_TILE; the top cell id has reads, n_cells - seen ids
    handed out have none."""
    rng = np.random.default_rng(n_cells)
    cells = np.concatenate((rng.choice(n_cells - 1, seen - 1, replace=False), [n_cells - 1]))
    st = _random_stream(rng, cells, 3 * seen, 4)
    exp = st.expected()
    tr, n_ecs = exp[0], exp[1]
    sizes = _triples_per_ec(tr, n_ecs)
    assert sizes.max() > SMALL and sizes.min() <= SMALL               # (small and big ECs both)
    with _builder(st, device) as b:
        a = _check_built(b, st, exp)
        totals = np.bincount(tr["cell"], weights=tr["count"], minlength=n_cells)
        for mc in (-1, int(np.median(totals[cells])) + 1):
            kept = _check_filter(b, a, tr, n_ecs, n_cells, mc)
            assert 0 < len(kept) <= seen
        f = b.ms_filter(n_cells, 1)
        assert f["n_cells_seen"] == seen and len(f["kept_cells"]) == seen and n_cells - 1 in f["kept_cells"]


def test_n_cells_out_of_range_is_refused():
    st = _in_file_order(np.random.default_rng(0), [0, 1, 0], [0, 1, 2], [0, 0, 1])
    with _builder(st) as b:
        _check_built(b, st, st.expected())
        for bad in (0, MAX_CELLS + 1):
            with pytest.raises(ecb.EcbError) as e:
                b.ms_filter(bad, 1)
            assert e.value.code == -1


# ---- ECs on the thread / workgroup / grid limits, the edges of the meta word ------------------------------------------------------
def _edge_stream():
    """ECs of exactly 1, 256, 257, 32 768 and 32 769 triples, giant ECs of 40 000 and 1.1 M triples, 300 small ECs; cells over all of
    0 .. 2^22 - 1 and files over 0 .. 1023.  Cell 2^22 - 1 has reads in file 1023 (meta 0xFFFFFFFF); cell 12345 only in files 5 and
    700; cell 777 has the reads of one small EC in 600 files, cell 4242 those of the largest EC in 400 files (the pairs
    k_msf2_pairs adds up)."""
    rng = np.random.default_rng(4)
    exact = [1, SMALL, SMALL + 1, GIANT, GIANT + 1, 40_000, 1_100_000]
    filler = rng.integers(1, 60, 300)
    want = list(exact) + list(filler)
    pool = np.unique(rng.integers(0, 1 << 32, int(sum(want) * 1.05), dtype=np.uint64).astype(np.int64))
    pool = pool[rng.permutation(len(pool))]
    tpl, pair, at = [], [], 0
    for k, n in enumerate(want):                                      # template k: n distinct (cell, file) pairs
        tpl.append(np.full(n, k)); pair.append(pool[at:at + n]); at += n
    big = len(exact) - 1
    special = [(len(exact), np.arange(600), 777), (big, np.arange(400) * 2 + 3, 4242), (len(exact) + 1, np.array([5, 700]), 12345),
               (len(exact) + 2, np.array([1023]), MAX_CELLS - 1), (len(exact) + 2, np.array([0, 1023]), 0)]
    for k, files, c in special:
        tpl.append(np.full(len(files), k)); pair.append((np.int64(c) << 10) | files)
    tpl, pair = np.concatenate(tpl), np.concatenate(pair)
    # other ECs' cells 777, 4242, 12345, 2^22 - 1 and 0 appear only where placed above
    _, i = np.unique((tpl << 32) | pair, return_index=True)
    tpl, pair = tpl[i], pair[i]
    cell, fil = pair >> 10, pair & 1023
    placed = np.isin(cell, [777, 4242, 12345, MAX_CELLS - 1, 0])
    mine = np.zeros(len(tpl), bool)
    for k, files, c in special:
        mine |= (tpl == k) & (cell == c) & np.isin(fil, files)
    keep = ~placed | mine
    tpl, cell, fil = tpl[keep], cell[keep], fil[keep]
    reads = 1 + (rng.random(len(tpl)) < 0.2) * rng.integers(1, 4, len(tpl))          # reads per triple
    reads[cell == 4242] = 2                                                           # cell 4242: 800 reads
    reads[cell == 777] = 2                                                            # cell 777: 1 200 reads, the most of any cell
    return _in_file_order(rng, np.repeat(tpl, reads), np.repeat(cell, reads), np.repeat(fil, reads)), exact


@pytest.fixture(scope="module")
def edge():
    st, exact = _edge_stream()
    exp = st.expected()
    return st, exact, exp


def test_ecs_on_the_thread_workgroup_and_grid_limits_and_every_meta_edge(edge):
    st, exact, exp = edge
    tr, n_ecs = exp[0], exp[1]
    sizes = _triples_per_ec(tr, n_ecs)
    for n in exact[:5]:
        assert n in sizes.tolist(), n
    assert (sizes > GIANT).sum() >= 3 and sizes.max() > 10**6            # gfec rows g > 0
    m = tr["cell"] | (tr["file"] << CELL_BITS)
    assert m.max() == 0xFFFFFFFF and tr["file"].min() == 0
    assert set(tr["file"][tr["cell"] == 12345].tolist()) == {5, 700}
    per = {}
    for e, c in zip(tr["ec"].tolist(), tr["cell"].tolist()):
        if c in (777, 4242):
            per[(e, c)] = per.get((e, c), 0) + 1
    assert sorted(per.values())[-2:] == [400, 600]                        # (EC, cell) pairs over hundreds of files
    totals = np.bincount(tr["cell"], weights=tr["count"], minlength=MAX_CELLS).astype(np.int64)
    top = np.sort(totals)[::-1]
    assert totals[777] == top[0] > top[1] == totals[4242] > top[2]
    with _builder(st) as b:
        a = _check_built(b, st, exp)
        for mc in (-1, 0, 1):
            assert len(_check_filter(b, a, tr, n_ecs, MAX_CELLS, mc)) == (totals > 0).sum()
        assert sorted(_check_filter(b, a, tr, n_ecs, MAX_CELLS, int(totals[4242]))) == [777, 4242]     # exactly one cell's total
        assert _check_filter(b, a, tr, n_ecs, MAX_CELLS, int(totals[4242]) + 1) == [777]    # keeps exactly one cell
        assert _check_filter(b, a, tr, n_ecs, MAX_CELLS, int(totals[777])) == [777]
        assert _check_filter(b, a, tr, n_ecs, MAX_CELLS, int(totals[777]) + 1) == []        # keeps none: -7


# ---- one handle, several filters; reset ------------------------------------------------------------------------------------------
def test_one_handle_filtered_again_and_again_then_reset_for_another_stream():
    """Pool buffers are reused between filters: a large result, a smaller one, a larger one, each == the checker; then reset() and a
    different stream (LDS path after the global one) on the same handle."""
    rng = np.random.default_rng(11)
    st = _random_stream(rng, np.arange(9000), 60_000, 5)
    exp = st.expected()
    tr, n_ecs = exp[0], exp[1]
    totals = np.bincount(tr["cell"], weights=tr["count"], minlength=9000)
    q90 = int(np.quantile(totals, 0.9)) + 1
    with _builder(st) as b:
        a = _check_built(b, st, exp)
        n1 = len(_check_filter(b, a, tr, n_ecs, 9000, 1))
        n2 = len(_check_filter(b, a, tr, n_ecs, 9000, q90))
        n3 = len(_check_filter(b, a, tr, n_ecs, 9500, 2))
        assert n1 > n3 > n2 > 0
        b.reset()
        st2 = _random_stream(rng, np.arange(3000) * 2, 20_000, 3, n_tpl=700)
        exp2 = st2.expected()
        _push(b, st2)
        a2 = _check_built(b, st2, exp2)
        _check_filter(b, a2, exp2[0], exp2[1], 6000, -1)
        _check_filter(b, a2, exp2[0], exp2[1], 6000, 8)


# ---- the smallest inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tpl,cell,fil,n_cells", [
    ([0], [0], [0], 1),                                      # one read in one cell (the sorts return early at n < 2)
    ([3], [MAX_CELLS - 1], [1023], MAX_CELLS),              # one read, meta 0xFFFFFFFF
    ([0, 1], [1, 0], [0, 0], 2),                             # two cells, in the order their reads come
    ([0, 0, 1], [0, 1, 1], [0, 1, 1], 2),                    # two cells; cell 0's first file is file 0, cell 1's file 1
], ids=["one-read", "one-read-top-meta", "two-cells", "two-cells-two-files"])
def test_smallest_inputs(tpl, cell, fil, n_cells):
    st = Stream(tpl, cell, fil)
    exp = st.expected()
    with _builder(st) as b:
        a = _check_built(b, st, exp)
        for mc in (-1, 1, 2):
            _check_filter(b, a, exp[0], exp[1], n_cells, mc)


# ---- shards ----------------------------------------------------------------------------------------------------------------------
def _sharded(st, cuts, edit=None, extra_reads=0):
    """The multi-GPU protocol of alntools_amd/dist.py on one card, as test_gpu_parity.py::test_multisample_over_shards_equals_one_handle
    runs it: contiguous read shards, tables merged by key range and adopted by a multisample root, triples looked up by every shard
    (ms_local_triples) and combined on the root (ms_adopt_triples).  ``edit(tables)`` may change the shards' triples before they are
    adopted; ``extra_reads`` are added to the root's read total.  -> root engine (finalized, triples adopted), shard handles."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    shards, pieces, sizes, base = [], [], [], 0
    P = len(cuts) - 1
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        b = ecb.EcBuilder(st.n_loci, H, ec_capacity=1 << 12, multisample=True)
        b.push(*st.records(r0, r1))
        b.push_cells(st.meta[r0:r1], 0)
        eng = ecdist.GpuEngine(b, dev)
        nreads = b.table_sizes()[2]
        assert nreads == r1 - r0
        pieces.append(eng.table_export_parts(base, P))
        sizes.append((nreads,) + b.counters()[:2])
        shards.append((eng, base))
        base += nreads
    root = ecdist.GpuEngine(ecb.EcBuilder(st.n_loci, H, ec_capacity=1 << 12, multisample=True), dev)
    adopted = []
    for q in range(P):
        part = ecdist.GpuEngine(ecb.EcBuilder(st.n_loci, H, ec_capacity=1 << 12), dev)
        part.table_merge_many([(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                               for ent, prs, eoff, poff in pieces if eoff[q + 1] > eoff[q]])
        pe_n, pp_n, _ = part.table_sizes()
        adopted.append(part.table_export(0) + (pe_n, pp_n))
        part.b.close()
    root.table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
    root.add_counters(sum(s[1] for s in sizes) + extra_reads, sum(s[2] for s in sizes) + extra_reads, base + extra_reads)
    s = root.b.finalize()
    keys, nnz = root.ec_keys(s["n_ecs"])
    tables = [eng.ms_local_triples(keys, s["n_ecs"], nnz, b0) for eng, b0 in shards]
    if edit is not None:
        edit(tables)
        torch.cuda.synchronize()                                  # (libecb works on its own stream)
    root.ms_adopt_triples(tables)
    return root, [eng.b for eng, _ in shards]


def test_multisample_over_shards_with_extreme_metas_equals_one_handle():
    """Shards whose cells (more than 8 192, and cell 2^22 - 1 in file 1023) straddle the cuts: root export_pairs and ms_filter
    == one handle over the whole stream == the checker."""
    rng = np.random.default_rng(21)
    cells = np.concatenate((np.arange(12_000) * 37, [MAX_CELLS - 1]))
    st = _random_stream(rng, cells, 80_000, 1024, n_tpl=1500, pinned=[(MAX_CELLS - 1, 1023)])
    assert st.meta.max() == 0xFFFFFFFF
    exp = st.expected()
    tr, n_ecs = exp[0], exp[1]
    cuts = [0, 23_456, 50_001, st.n_reads]
    for k in range(1, 3):                                         # cells on both sides of each cut
        c = cuts[k]
        assert len(np.intersect1d(st.cell[:c], st.cell[c:])) > LDS_CELLS // 4
    root, shards = _sharded(st, cuts)
    try:
        got = root.b.export_pairs()
        for k in ("ec", "cell", "file", "count", "first"):
            assert np.array_equal(got[k], tr[k]), k
        a = root.b.export()
        with _builder(st) as one:
            a1 = _check_built(one, st, exp)
            for k in ("indptrA", "indicesA", "dataA"):
                assert np.array_equal(a[k], a1[k]), k
            for mc in (-1, 3):
                kept = _check_filter(root.b, a, tr, n_ecs, MAX_CELLS, mc)
                f1, f2 = one.ms_filter(MAX_CELLS, mc), root.b.ms_filter(MAX_CELLS, mc)
                assert f1["kept_cells"].tolist() == f2["kept_cells"].tolist() == kept
                for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN"):
                    assert np.array_equal(f1[k], f2[k]), k
                assert len(kept) > LDS_CELLS
    finally:
        root.b.close()
        for b in shards:
            b.close()


# ---- contract: cell ids not below n_cells ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells_used,n_cells_short", [(5000, 4000), (20_000, 10_000)], ids=["lds", "global"])
def test_cell_id_not_below_n_cells_is_refused_and_the_handle_stays_usable(n_cells_used, n_cells_short):
    """Cells up to n_cells_used - 1 filtered with n_cells = n_cells_short: ECB_ERR_CONTRACT (-5) -- with such triples in small, big and
    giant ECs, all of which pass them over -- and then the right n_cells on the same handle gives the right result."""
    rng = np.random.default_rng(n_cells_used)
    st = _random_stream(rng, np.arange(n_cells_used), 200_000, 16)
    exp = st.expected()
    tr, n_ecs = exp[0], exp[1]
    sizes = _triples_per_ec(tr, n_ecs)
    bad_ecs = np.unique(tr["ec"][tr["cell"] >= n_cells_short])
    assert (sizes[bad_ecs] <= SMALL).any() and ((sizes[bad_ecs] > SMALL) & (sizes[bad_ecs] <= GIANT)).any() and (sizes[bad_ecs] > GIANT).any()
    with _builder(st) as b:
        a = _check_built(b, st, exp)
        _check_filter(b, a, tr, n_ecs, n_cells_used, 5)
        with pytest.raises(ecb.EcbError) as e:
            b.ms_filter(n_cells_short, 1)
        assert e.value.code == -5
        assert b._lib.ecb_ms_export(b._h, *[None] * 7) == -6             # (the result before is gone: nothing stale to export)
        _check_filter(b, a, tr, n_ecs, n_cells_used, -1)
        _check_filter(b, a, tr, n_ecs, n_cells_used, 12)


# ---- int32 limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [I32, I32 + 1], ids=["2^31-1", "2^31"])
def test_entry_of_n_at_the_int32_limit(target):
    """One (EC, cell) pair whose reads sit in two files of the first shard, its counts raised (after ms_local_triples) to add up to
    ``target``: 2^31 - 1 is kept exactly in dataN; 2^31 is refused with ECB_ERR_LIMIT (-8), not wrapped.  The root's read total
    takes the added reads (below 2^32 - 1)."""
    import torch
    rng = np.random.default_rng(31)
    st = _random_stream(rng, np.arange(400), 20_000, 4, n_tpl=300)
    cuts = [0, 12_000, st.n_reads]
    exp = st.expected()
    tr, n_ecs = exp[0], exp[1]
    # a pair with exactly two files, all of its reads in shard 0
    pk = (st.ec_of_read()[0] << 22) | st.cell
    in1 = np.unique(pk[cuts[1]:])
    tk = (tr["ec"] << 22) | tr["cell"]
    u, nfile = np.unique(tk, return_counts=True)
    ok = u[(nfile == 2) & ~np.isin(u, in1)]
    assert len(ok)
    e, c = int(ok[0] >> 22), int(ok[0] & (MAX_CELLS - 1))
    sel = np.flatnonzero(tk == ok[0])
    orig = int(tr["count"][sel].sum())
    counts = [1 << 30, target - (1 << 30)]
    files = tr["file"][sel].tolist()

    def edit(tables):
        key, cnt, _, n = tables[0]
        k = key[:n]
        for f, v in zip(files, counts):
            hit = torch.nonzero(k == ((e << 32) | (f << CELL_BITS) | c)).flatten()
            assert hit.numel() == 1
            cnt[hit] = v

    root, shards = _sharded(st, cuts, edit=edit, extra_reads=target - orig)
    try:
        assert root.b.sizes["n_reads"] == st.n_reads + target - orig < (1 << 32) - 1
        tr2 = dict(tr)
        tr2["count"] = tr["count"].copy()
        tr2["count"][sel] = counts
        got = root.b.export_pairs()
        for k in ("ec", "cell", "file", "count", "first"):
            assert np.array_equal(got[k], tr2[k]), k
        if target > I32:
            with pytest.raises(ecb.EcbError) as er:
                root.b.ms_filter(400, -1)
            assert er.value.code == -8
            return
        a = root.b.export()
        f = root.b.ms_filter(400, -1)
        assert int(f["dataN"].max()) == I32
        _check_filter(root.b, a, tr2, n_ecs, 400, -1)
    finally:
        root.b.close()
        for b in shards:
            b.close()


@pytest.mark.parametrize("target", [I32, I32 + 1], ids=["2^31-1", "2^31"])
def test_single_sample_count_at_the_int32_limit_through_assemble_ranges(target):
    """A finalized piece whose first EC's count is raised to ``target`` and assembled (ecb_assemble_ranges_device): 2^31 - 1 comes
    out exactly in dataN, 2^31 (as the uint32 a count is) is refused with ECB_ERR_LIMIT (-8)."""
    import torch
    rng = np.random.default_rng(5)
    st = _random_stream(rng, np.arange(10), 5000, 1, n_tpl=200)
    exp = st.expected()
    n_ecs, (ip, ix, da) = exp[1], exp[2]
    with ecb.EcBuilder(st.n_loci, H) as b:
        b.push(st.read_id, st.locus, st.hapflag)
        s = b.finalize()
        ref = b.export()
        assert s["n_ecs"] == n_ecs
        assert np.array_equal(ref["indptrA"], ip) and np.array_equal(ref["indicesA"], ix) and np.array_equal(ref["dataA"], da)
        assert np.array_equal(ref["dataN"], np.bincount(st.ec_of_read()[0], minlength=n_ecs))
        nnz = s["nnz_a"]
        d = dict(ip=torch.empty(n_ecs + 1, dtype=torch.int32, device="cuda"), ix=torch.empty(nnz, dtype=torch.int32, device="cuda"),
                 da=torch.empty(nnz, dtype=torch.int32, device="cuda"), cn=torch.empty(n_ecs, dtype=torch.int32, device="cuda"),
                 fi=torch.empty(n_ecs, dtype=torch.int32, device="cuda"))
        b.export_piece_device(d["ip"], d["ix"], d["da"], d["cn"], d["fi"])
        all_al, valid, _ = b.counters()
    orig = int(ref["dataN"][0])
    d["cn"][0] = int(np.array(target, np.uint32).view(np.int32))         # (a count is a uint32 in an int32 slot)
    torch.cuda.synchronize()
    extra = target - orig
    with ecb.EcBuilder(st.n_loci, H) as r:
        piece = [(d["ip"], d["ix"], d["da"], d["cn"], d["fi"], n_ecs, nnz)]
        if target > I32:
            with pytest.raises(ecb.EcbError) as er:
                r.assemble_ranges_device(piece, st.n_reads + extra, all_al + extra, valid + extra)
            assert er.value.code == -8
            return
        s2 = r.assemble_ranges_device(piece, st.n_reads + extra, all_al + extra, valid + extra)
        assert s2["n_ecs"] == n_ecs and s2["n_reads"] == st.n_reads + extra
        out = r.export()
    want = ref["dataN"].astype(np.int64)
    want[0] = target
    assert np.array_equal(out["dataN"].astype(np.int64), want) and int(out["dataN"][0]) == I32
    for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN"):
        assert np.array_equal(out[k], ref[k]), k


def test_push_cells_beyond_the_read_limit_is_refused():
    """ecb_push_cells and ecb_push_cells_device both refuse reads beyond 2^32 - 2 (ECB_ERR_LIMIT) before they size anything."""
    import torch
    with ecb.EcBuilder(16, H, multisample=True) as b:
        for first, n in (((1 << 32) - 2, 1), ((1 << 32) - 1, 1), ((1 << 32) - 10, 9)):
            with pytest.raises(ecb.EcbError) as e:
                b.push_cells(np.zeros(n, np.uint32), first)
            assert e.value.code == -8, (first, n)
            d = torch.zeros(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(ecb.EcbError) as e:
                b.push_cells_device(d, first)
            assert e.value.code == -8, (first, n)
        st = Stream([0, 1], [0, 1], [0, 0])                       # the handle still works
        _push(b, st)
        exp = st.expected()
        a = _check_built(b, st, exp)
        _check_filter(b, a, exp[0], exp[1], 2, 1)
