"""Inputs placed exactly on the constants where a GPU kernel changes path, each against an independent reference (the C oracle, numpy /
scipy, ``ec_merge_checker`` or ``gt_checker``), bit for bit.  The constants are pinned by ``test_threshold_constants.py`` (CPU): a retune
that moves one fails there first and names the case here to update.

Values assumed (``alntools_amd/csrc``): ``k_stream.inc`` CMAX = 80 (ks_std / ks_par) or 64 (ks_short), WMAXR = 64 or 128; ``ecb.hip``
WT = 64 * RPL = 512 records per tile, SLOW_LDS = 4096, INL = 5, RANKED_MAX = 16, BIG_LDS = 2048, CVU_PIECE = 1536, CVU_MAX = 3072,
QSTRIPES = 64.

Which reads k_stream hands to k_slow: a pass is flushed behind a tile (before the batch's last tile) whenever the next tile would bring
more records than the pass table has room for (``n_ent + n_mine > WT + CMAX``), which in a stream of mostly distinct loci is behind every
tile; the read that is open there -- the one holding the tile's last record, even when that record is its last: the kernel sees the next
head only in the next tile -- carries its entries (distinct loci) into the next pass, and goes to k_slow when they are more than CMAX.
``verify_device``'s second figure counts the reads the exactness pass (ks_std) sent there."""
import numpy as np
import pytest

from alntools_amd import bin_utils, ecb
from oracle import c_oracle
from oracle import ec_oracle as orc

import ec_merge_checker as chk
import gt_checker
from test_gpu_parity import _check, _run_host

pytestmark = pytest.mark.gpu

WT = 512
CMAX_STD, CMAX_SHORT = 80, 64
SLOW_LDS = 4096
KNOBS = ("ECB_NO_PAR", "ECB_FORCE_PAR", "ECB_FORCE_SHORT", "ECB_NO_SHORT")
# compilation forced -> (environment, hint the stream's reads, name ecb_profile_kernel reports)
COMPILATIONS = {"std": (("ECB_NO_PAR",), False, "ks_std::"), "par": (("ECB_FORCE_PAR",), False, "ks_par::"),
                "short": (("ECB_FORCE_SHORT",), True, "ks_short::"), "std_hinted": (("ECB_NO_SHORT", "ECB_NO_PAR"), True, "ks_std::")}


def _stream(reads):
    """reads: list of (loci, haps[, flags]) arrays, one read each, in order -> tuple dict (read ids 0, 1, ...)."""
    rid = np.concatenate([np.full(len(r[0]), k, np.uint32) for k, r in enumerate(reads)])
    loc = np.concatenate([np.asarray(r[0], np.uint32) for r in reads])
    hap = np.concatenate([np.asarray(r[1], np.uint32) for r in reads])
    flg = np.concatenate([np.asarray(r[2], np.uint32) if len(r) > 2 else np.zeros(len(r[0]), np.uint32) for r in reads])
    return dict(read_id=rid, locus=loc, hapflag=(flg | (hap << 16)).astype(np.uint32), pos=np.zeros(len(rid), np.int32))


def _distinct(rng, n, T, H):
    """A read of n records on n distinct loci (a run of consecutive target ids, as aligners give them)."""
    base = int(rng.integers(0, T - n))
    return base + np.arange(n), rng.integers(0, H, size=n)


def _fill(rng, n, T, H):
    """n records of short reads (1 .. 9 records each, distinct loci within a read)."""
    out = []
    while n > 0:
        k = min(n, int(rng.integers(1, 10)))
        out.append(_distinct(rng, k, T, H))
        n -= k
    return out


def _oracle(t, H):
    return c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=4)


def _dev(t):
    import torch
    return [torch.from_numpy(t[k].view(np.int32)).cuda() for k in ("read_id", "locus", "hapflag")]


def _force(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in env or ():
        monkeypatch.setenv(k, "1")


def _every_push(t, T, H, exp, monkeypatch, batches=(333, 4097), n_long=None):
    """The stream through every compilation (forced, each reported by ecb_profile_kernel) in one device push and as whole tiles, through
    the host push in odd batch sizes, and the exactness pass: == exp.  n_long: (least, most) reads the pass may send to k_slow."""
    d = _dev(t)
    n = len(t["read_id"])
    tiles = ecb.tile_tuples(*d)
    for name, (env, hinted, kernel) in COMPILATIONS.items():
        _force(monkeypatch, env)
        with ecb.EcBuilder(T, H) as b:
            if hinted:
                b.hint_reads(exp["n_reads"])
            b.push_device(*d)
            assert b.profile_kernel().startswith(kernel), (name, b.profile_kernel())
            _check(b.export(), b.finalize(), exp)
            b.reset()
            if hinted:
                b.hint_reads(exp["n_reads"])
            b.push_device_tiled(tiles, n)
            assert b.profile_kernel().startswith(kernel), (name, b.profile_kernel())
            _check(b.export(), b.finalize(), exp)
            b.reset()
            b.push_device(*d)
            bad, long_ = b.verify_device(*d)
            assert bad == 0, name
            if n_long is not None:
                assert n_long[0] <= long_ <= n_long[1], (name, long_, n_long)
    _force(monkeypatch, None)
    for batch in batches:
        out, sizes = _run_host(t, T, H, batch=batch)
        _check(out, sizes, exp)


def _carry_stream(cmax, n_tiles, seed):
    """Tile after tile, a read that holds the tile's last records: k = cmax - 1, cmax or cmax + 1 distinct loci before the tile's end (with
    or without one duplicate record among them -- same locus, another haplotype: records != loci), then nothing more (it ends on the tile's
    end: open there all the same), one duplicate record, or one new locus in the next tile.  -> (tuples, reads ks_std must defer)."""
    rng = np.random.default_rng(seed)
    T, H = 100_000, 4
    reads, at, giants = [], 0, 0
    for t in range(n_tiles):
        k = cmax - 1 + t % 3
        dup = (t // 3) % 2
        tail = (t // 6) % 3
        end = (t + 1) * WT
        pre = k + dup
        reads += _fill(rng, end - pre - at, T, H)
        loci, haps = _distinct(rng, k, T, H)
        if dup:
            j = k // 2
            loci = np.insert(loci, j + 1, loci[j])
            haps = np.insert(haps, j + 1, (haps[j] + 1) % H)
        if tail == 1:
            loci, haps = np.append(loci, loci[0]), np.append(haps, (haps[0] + 1) % H)
        elif tail == 2:
            loci, haps = np.append(loci, loci[-1] + 1), np.append(haps, 0)
        reads.append((loci, haps))
        at = end + (tail != 0)
        giants += k > CMAX_STD
    reads += _fill(rng, (n_tiles + 1) * WT + 100 - at, T, H)          # (the last tile ends the batch: no flush with a read open)
    return _stream(reads), T, H, giants


@pytest.mark.parametrize("cmax", [CMAX_STD, CMAX_SHORT])
def test_reads_carrying_cmax_and_one_more_entries_over_a_tile_end(cmax, monkeypatch):
    """CMAX (``k_stream.inc:30``): a read open at a flush with CMAX entries is carried, with CMAX + 1 it goes to k_slow (``giant``,
    ``k_stream.inc:681``).  Streams built tile by tile so that the open read holds CMAX - 1, CMAX and CMAX + 1 distinct loci at the tile's
    end, against the C oracle in every compilation and push.  The exactness pass (ks_std, CMAX 80) defers none of the reads carrying 63,
    64, 65, 79 or 80 entries, and some (not all: a flush is not certain behind every tile) of the twelve carrying 81."""
    t, T, H, giants = _carry_stream(cmax, 36, 100 + cmax)
    exp = _oracle(t, H)
    assert giants == (12 if cmax == CMAX_STD else 0)
    _every_push(t, T, H, exp, monkeypatch, n_long=(1, giants) if giants else (0, 0))


def test_reads_of_a_whole_tile_and_tiles_of_many_reads(monkeypatch):
    """WT = 64 * RPL = 512 (``ecb.hip: WT``) and WMAXR = 64 / 128 (``k_stream.inc:17``): reads of exactly 512 records that start on a tile
    start and one record before it, on distinct loci (open at the tile end with 512 entries: deferred) and on 40 loci repeated (carried);
    tiles of 65, 129 and 200 one-record reads (more than a pass of either kernel takes: the tile is visited again); and a read of 2 600
    records, longer than a slice.  The slice size is not in the ABI: ``plan_stream`` (``ecb.hip: plan_stream``) cuts n records into
    min(resident waves x 24, max(n / (32 x 512), resident waves), ceil(n / 1024)) slices of ceil(n / slices) records rounded up to whole
    tiles; with 26 k records and the thousands of waves an MI355X holds that is ceil(n / 1024) slices of 1 024 records, so the read spans two
    whole slices and the slice after them starts inside it."""
    rng = np.random.default_rng(7)
    T, H = 50_000, 8
    reads, at = [], 0

    def pad_to(x):
        nonlocal at
        reads.extend(_fill(rng, x - at, T, H))
        at = x

    def add(loci, haps):
        nonlocal at
        reads.append((loci, haps))
        at += len(loci)
    pad_to(WT)
    add(*_distinct(rng, WT, T, H))                                   # tile 1, exactly: open at its end with 512 entries
    pad_to(3 * WT - 1)
    add(*_distinct(rng, WT, T, H))                                   # one record before tile 3 .. one record before tile 4
    pad_to(5 * WT)
    add((rng.integers(0, 40, WT) * 3 + 1000), rng.integers(0, H, WT))     # 512 records on <= 40 loci: carried, never deferred
    pad_to(7 * WT - 1)
    add((rng.integers(0, 40, WT) * 3 + 2000), rng.integers(0, H, WT))
    for nr in (65, 129, 200):                                        # tiles of more reads than WMAXR
        pad_to((at + WT - 1) // WT * WT)
        for _ in range(nr):
            add(*_distinct(rng, 1, T, H))
    pad_to((at + WT - 1) // WT * WT + 300)
    add(*_distinct(rng, 2600, T, H))                                 # longer than a slice (1 024 records)
    pad_to(at + 9000)
    t = _stream(reads)
    exp = _oracle(t, H)
    _every_push(t, T, H, exp, monkeypatch, batches=(511, 1023, 5000))


@pytest.mark.parametrize("distinct", [True, False])
def test_k_slow_lds_limit(distinct, monkeypatch):
    """SLOW_LDS = 4096 (``ecb.hip: SLOW_LDS``): k_slow keeps a read's table in LDS when 2 x its records <= SLOW_LDS (``ecb.hip: k_slow``), so reads of
    2 047 and 2 048 records take the LDS body and 2 049 the global one.  All loci distinct, or 700 loci repeated round (every whole tile of
    such a read holds 512 distinct loci: open at the tile's end with more than CMAX entries, so all six are deferred).  Host and device
    pushes against the C oracle; the exactness pass sends exactly those six reads to k_slow."""
    rng = np.random.default_rng(11 + distinct)
    T, H = 20_000, 8
    reads = []
    for L in (2047, 2048, 2049, 2049, 2048, 2047):
        reads += _fill(rng, int(rng.integers(1, 700)), T, H)
        if distinct:
            reads.append(_distinct(rng, L, T, H))
        else:
            base = int(rng.integers(0, T - 700))
            reads.append((base + np.arange(L) % 700, rng.integers(0, H, L)))
    reads += _fill(rng, 3000, T, H)
    t = _stream(reads)
    exp = _oracle(t, H)
    assert sorted(np.bincount(t["read_id"].astype(np.int64)))[-6:] == [2047, 2047, 2048, 2048, 2049, 2049]
    d = _dev(t)
    with ecb.EcBuilder(T, H) as b:
        b.push_device(*d)
        _check(b.export(), b.finalize(), exp)
        b.reset()
        b.push_device(*d)
        assert b.verify_device(*d) == (0, 6)
    for batch in (None, 1999):
        out, sizes = _run_host(t, T, H, batch=batch)
        _check(out, sizes, exp)


@pytest.mark.parametrize("compilation", ["std", "short"])
def test_every_read_deferred(compilation, monkeypatch):
    """QSTRIPES = 64 (``ecb.hip: QSTRIPES``): the deferred-read queue is 64 hash-picked stripes of need_q / 64 heads, need_q = pwaves x (WT + 1) +
    n / 64 + 16 (``ecb.hip: need_q``), and a full stripe is fatal.  A launch defers at most one read per tile end (the one open there), so no
    stream defers more than n / 512 reads.  Here every read does: 12 M records in reads of 2 x WT + 1 = 1 025 distinct loci -- each covers a
    whole tile and is still open at its end, holding 512 entries > CMAX -- 11 707 deferred reads through ks_std and (forced) ks_short, one
    device push, against the C oracle.  (Passed as the queue stood: 183 heads a stripe on average against 4 k and more of room.)"""
    import torch
    R, Lr, T, H = 11_707, 2 * WT + 1, 60_000, 4
    rng = np.random.default_rng(5)
    base = rng.integers(0, T - Lr, size=R)
    loc = (base[:, None] + np.arange(Lr)[None, :]).reshape(-1).astype(np.uint32)
    t = dict(read_id=np.repeat(np.arange(R, dtype=np.uint32), Lr), locus=loc,
             hapflag=(rng.integers(0, H, size=R * Lr).astype(np.uint32) << 16))
    assert len(loc) > 10_000_000
    exp = _oracle(t, H)
    d = _dev(t)
    env, hinted, kernel = COMPILATIONS[compilation]
    _force(monkeypatch, env)
    with ecb.EcBuilder(T, H) as b:
        if hinted:
            b.hint_reads(R)
        b.push_device(*d)
        assert b.profile_kernel().startswith(kernel)
        _check(b.export(), b.finalize(), exp)
        b.reset()
        b.push_device(*d)
        assert b.verify_device(*d) == (0, R)
    del d
    torch.cuda.empty_cache()


def _key_reads(rng, T, H, sizes):
    """One read per key length in `sizes` (distinct loci in a random order, one duplicate record with another haplotype)."""
    reads = []
    for n in sizes:
        loci = np.sort(rng.choice(T, size=n, replace=False))
        haps = rng.integers(0, H, n)
        o = rng.permutation(n)
        reads.append((np.append(loci[o], loci[o[0]]), np.append(haps[o], (haps[o[0]] + 1) % H)))
    return reads


KEY_SIZES = (4, 5, 6, 15, 16, 17, 2047, 2048, 2049, 5003)


def test_key_lengths_through_finalize_merge_adopt_and_ecb_merge():
    """INL = 5 (``ecb.hip: INL``: pairs held in the table slot), RANKED_MAX = 16 (``ecb.hip: RANKED_MAX``: keys of more go one wave each through
    export and emit) and BIG_LDS = 2048 (``ecb.hip: BIG_LDS``: keys of more are walked in memory by the emit and k_parts_sort_big): ECs of
    4/5/6, 15/16/17, 2047/2048/2049 and 5003 pairs, each read twice or three times, in contiguous read shards that share ECs.  One handle
    over the whole stream (host and device push) against the C oracle; 2 and 3 shards on one GPU through table_export_parts ->
    table_merge_batch_device -> table_adopt_device and through ecb_merge (EcBuilder.merge_from), each == the oracle."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    T, H = 8000, 8
    keys = _key_reads(rng, T, H, KEY_SIZES)
    order = list(range(len(keys))) + [9, 8, 7, 6, 5, 4, 3, 2, 1, 0] + [2, 5, 8, 7]
    t = _stream([keys[i] for i in order])
    exp = _oracle(t, H)
    assert sorted(np.diff(exp["indptr"]).tolist()) == sorted(KEY_SIZES)
    out, sizes = _run_host(t, T, H, batch=3001)
    _check(out, sizes, exp)
    d = _dev(t)
    with ecb.EcBuilder(T, H) as b:
        b.push_device(*d)
        _check(b.export(), b.finalize(), exp)
    rid = t["read_id"]
    for cut_reads in ([0, 12, len(order)], [0, 7, 15, len(order)]):
        cuts = [int(np.searchsorted(rid, r)) for r in cut_reads]

        def shards():
            out = []
            for a, z in zip(cuts[:-1], cuts[1:]):
                b = ecb.EcBuilder(T, H, ec_capacity=1 << 10)
                b.push(t["read_id"][a:z] - t["read_id"][a], t["locus"][a:z], t["hapflag"][a:z])
                out.append(b)
            return out
        # the multi-GPU protocol by key range, on one card
        P = len(cuts) - 1
        pieces, counts, base = [], [], 0
        for b in shards():
            nreads = b.table_sizes()[2]
            pieces.append(ecdist.GpuEngine(b, dev).table_export_parts(base, P))
            counts.append(b.counters()[:2])
            base += nreads
            b.close()
        root = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 10), dev)
        for q in range(P):
            part = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 10), dev)
            part.table_merge_many([(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q])
                                   for ent, prs, eo, po in pieces if eo[q + 1] > eo[q]])
            pe_n, pp_n, _ = part.table_sizes()
            pe, pp = part.table_export(0)
            root.table_adopt(pe, pe_n, pp, pp_n)
            part.b.close()
        root.add_counters(sum(c[0] for c in counts), sum(c[1] for c in counts), base)
        _check(root.b.export(), root.b.finalize(), exp)
        root.b.close()
        # ... and inside the library
        sh = shards()
        with ecb.EcBuilder(T, H, ec_capacity=1 << 10) as r2:
            s = r2.merge_from(sh)
            _check(r2.export(), s, exp)
        for b in sh:
            b.close()


def test_ranges_min_max_and_sentinel_on_the_stream_and_k_slow_paths():
    """ECB_F_RANGES: ``export_ranges`` and ``export_range_minmax`` (the multi-rank ``--rangefile`` path) against numpy's per-(locus,
    haplotype) min / max of reference_start over valid records.  Untouched slots keep k_fill_minmax's (INT_MAX, INT_MIN) and a range of 0;
    positions 0 and 2^31 - 2; pairs seen once; a pair seen only by invalid records; reads of 2 x WT + 1 distinct loci (deferred to k_slow)
    beside short ones.  Host pushes in two batch sizes and one device push."""
    import torch
    rng = np.random.default_rng(31)
    T, H = 4000, 4
    reads = []
    for k in range(400):
        if k % 40 == 7:
            loci, haps = _distinct(rng, 2 * WT + 1, T - 10, H)
        else:
            loci, haps = _distinct(rng, int(rng.integers(1, 12)), T - 10, H)
        flags = np.where(rng.random(len(loci)) < 0.1, 0x4, 0).astype(np.uint32)
        flags[0] = 0
        reads.append((loci, haps, flags))
    reads.append((np.array([T - 5, T - 5, T - 3]), np.array([0, 1, 2]), np.array([0, 0x4, 0])))       # (T-5, 1): invalid records only
    reads.append((np.array([T - 2]), np.array([3]), np.array([0])))                                     # seen once
    t = _stream(reads)
    n = len(t["read_id"])
    pos = rng.integers(1, (1 << 31) - 2, size=n).astype(np.int64)
    pos[rng.integers(0, n, 40)] = 0
    pos[rng.integers(0, n, 40)] = (1 << 31) - 2
    t["pos"] = pos.astype(np.int32)
    valid = orc.tuples_valid(t["hapflag"])
    hap = (t["hapflag"].astype(np.int64) >> 16) & 0xFF
    slot = t["locus"].astype(np.int64) * H + hap
    mn = np.full(T * H, np.iinfo(np.int32).max, np.int64)
    mx = np.full(T * H, np.iinfo(np.int32).min, np.int64)
    np.minimum.at(mn, slot[valid], pos[valid])
    np.maximum.at(mx, slot[valid], pos[valid])
    length = np.where(mx == np.iinfo(np.int32).min, 0, mx - mn + 1)
    assert mn[(T - 5) * H + 1] == np.iinfo(np.int32).max and (mn == 0).any() and (mx == (1 << 31) - 2).any()
    assert length[(T - 2) * H + 3] == 1
    exp = _oracle(t, H)

    def check(b):
        _check(b.export(), b.finalize(), exp)
        assert np.array_equal(b.export_ranges().reshape(-1), length)
        gmn, gmx = b.export_range_minmax()
        assert np.array_equal(gmn.reshape(-1), mn) and np.array_equal(gmx.reshape(-1), mx)
    for batch in (None, 777):
        with ecb.EcBuilder(T, H, track_ranges=True) as b:
            step = batch or n
            for a in range(0, n, step):
                s = slice(a, a + step)
                b.push(t["read_id"][s], t["locus"][s], t["hapflag"][s], t["pos"][s])
            check(b)
    d = _dev(t) + [torch.from_numpy(t["pos"]).cuda()]
    with ecb.EcBuilder(T, H, track_ranges=True) as b:
        b.push_device(*d)
        assert b.profile_kernel() == "ks_std::k_stream<false, true>"
        check(b)


def _bin(rows, lname, hname, snames, counts):
    """ECMatrices from a list of (columns, masks) rows and a list per sample of {row: count}."""
    H = len(hname)
    ip = np.cumsum([0] + [len(r[0]) for r in rows])
    ix = np.concatenate([np.asarray(r[0], np.int64) for r in rows] + [np.zeros(0, np.int64)])
    dx = np.concatenate([np.asarray(r[1], np.int64) for r in rows] + [np.zeros(0, np.int64)])
    nip, nix, ndx = [0], [], []
    for c in counts:
        e = sorted(c)
        nix += e
        ndx += [c[k] for k in e]
        nip.append(len(nix))
    lengths = np.arange(len(lname) * H).reshape(len(lname), H) % 997 + 100
    return bin_utils.ECMatrices(hname, lname, lengths, snames, ip, np.array(ix, np.int64), np.array(dx, np.int64), nip,
                                np.array(nix, np.int64), np.array(ndx, np.int64))


def _combine(ms):
    plan = bin_utils.plan_merge(ms)
    parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                  n_loci=m.num_loci, target_map=tm, sample_map=sm) for m, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
    return bin_utils.ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname,
                                *ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname)))


@pytest.mark.parametrize("H", [1, 31])
def test_ecmerge_long_rows_one_and_31_haplotypes(H):
    """``ecb_combine`` with H = 1 and H = 31 (every mask with bit 30 set), rows of 2 047 / 2 048 / 2 049 (BIG_LDS = 2048, ``ecb.hip: BIG_LDS``)
    and 5 000 pairs in two parts that share them, one part under a shuffled target list, and a part whose rows are all empty: against
    ec_merge_checker."""
    rng = np.random.default_rng(40 + H)
    T = 6000
    lname = ["t%05d" % i for i in range(T)]
    hname = ["h%d" % i for i in range(H)]

    def row(n):
        cols = np.sort(rng.choice(T, size=n, replace=False))
        masks = np.ones(n, np.int64) if H == 1 else (rng.integers(0, 1 << 30, size=n) | (1 << 30))
        return cols, masks
    long_rows = [row(n) for n in (2047, 2048, 2049, 5000)]
    short = [row(int(rng.integers(1, 20))) for _ in range(30)]
    a_rows = long_rows + short[:15] + [(np.zeros(0, np.int64), np.zeros(0, np.int64))]
    b_rows = short[10:] + long_rows[::-1] + [row(2049)]
    a = _bin(a_rows, lname, hname, ["s1"], [{k: k + 1 for k in range(len(a_rows))}])
    b = _bin(b_rows, lname, hname, ["s1", "s2"], [{k: 2 for k in range(0, len(b_rows), 2)}, {k: 3 for k in range(len(b_rows))}])
    empty = _bin([(np.zeros(0, np.int64), np.zeros(0, np.int64))] * 3, lname, hname, ["s3"], [{0: 4, 2: 1}])
    for ms in ([a, b], [b, a], [a, chk.permute_targets(b, rng)], [a, empty, b], [empty]):
        got = _combine(ms)
        assert bin_utils.ecsave2_bytes(got) == chk.merge_bytes(ms)
        assert int(np.diff(got.indptrA).max()) == (5000 if ms[0] is not empty else 0)


def test_ecmerge_count_of_exactly_int32_max_is_accepted():
    """A merged count of 2^31 - 1 is written as it is; 2^31 is ECB_ERR_LIMIT (-8)."""
    lname, hname = ["a", "b", "c"], ["A", "B"]
    rows = [(np.array([0, 2]), np.array([1, 3])), (np.array([1]), np.array([2]))]
    top = (1 << 31) - 1
    a = _bin(rows, lname, hname, ["s"], [{0: top - 5, 1: 7}])
    b = _bin(rows[::-1], lname, hname, ["s"], [{1: 5, 0: 9}])
    got = _combine([a, b])
    assert got.dataN.tolist() == [top, 16]
    assert bin_utils.ecsave2_bytes(got) == chk.merge_bytes([a, b])
    c = _bin(rows, lname, hname, ["s"], [{0: 1}])                  # (EC 0: 2^31 - 6 + 1 + 5)
    with pytest.raises(ecb.EcbError) as e:
        _combine([a, c, b])
    assert e.value.code == -8


def test_apply_genotypes_long_rows_and_bit_30():
    """``ecb_apply_mask`` on rows of 2 049 - 5 000 loci (beyond BIG_LDS) among short ones, with H = 31 and a mask that keeps bit 30 only
    (zero elsewhere on a third of the loci): host and device entries against gt_checker."""
    import torch
    rng = np.random.default_rng(51)
    T, H = 7000, 31
    lens = [2049, 5000, 0, 3, 2050, 1, 4096] + list(rng.integers(0, 12, 300))
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ix = np.concatenate([np.sort(rng.choice(T, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    da = rng.integers(1, 1 << 31, size=len(ix), dtype=np.int64)
    da = np.where(rng.random(len(ix)) < 0.9, da | (1 << 30), da).astype(np.int32)            # (most keep their bit 30)
    for mask in (np.full(T, 1 << 30, np.int64), np.where(rng.random(T) < 0.33, 0, 1 << 30)):
        exp = gt_checker.mask_csr(ip, ix, da, mask)
        got = ecb.apply_mask(ip, ix, da, mask.astype(np.uint32), H)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)
        dg = ecb.apply_mask(*(torch.from_numpy(x).cuda() for x in (ip, ix, da)), torch.from_numpy(mask.astype(np.int32)).cuda(), H)
        for g, e in zip(dg, exp):
            assert np.array_equal(g.cpu().numpy(), e)
        assert (np.diff(exp[0]) > 2048).any()


@pytest.mark.parametrize("n_col", [2304, 2305, 3072, 3073])
def test_per_haplotype_csc_columns_on_the_piece_limits(n_col):
    """CVU_PIECE = 1536, CVU_MAX = 3072 (``ecb.hip: CVU_PIECE, CVU_MAX``): a column of more than 1.5 x CVU_PIECE = 2 304 row indices (summed over
    the haplotypes) is cut into ceil(n / 1536) pieces by EC range (``k_cvu_pieces``); a piece of more than CVU_MAX goes entry by entry
    (``ecb.hip: k_cvu_union``).  Columns of exactly 2 304 / 2 305 / 3 072 / 3 073 row indices over three haplotypes, with ECs spread over all ids
    and bunched into the first quarter (every index in the first piece: 3 072 fill the LDS table, 3 073 take the entry path), both
    directions on the device and on host arrays, against scipy.  (A piece of exactly 3 072 once sized its table at 8 192 slots of
    CVU_TSZ = 4 096 and came back with ECs listed twice.)"""
    import torch
    from scipy import sparse
    rng = np.random.default_rng(n_col)
    E, T, H = 40_000, 6, 3
    r, c, b = [], [], []
    for col, span in ((0, E), (1, E // 4), (2, E // 4)):
        split = [n_col // 3, n_col // 3, n_col - 2 * (n_col // 3)]
        for h in range(H):
            r.append(rng.choice(span, size=split[h], replace=False))
            c.append(np.full(split[h], col))
            b.append(np.full(split[h], h))
    for col in range(3, T):
        for h in range(H):
            k = int(rng.integers(0, 40))
            r.append(rng.choice(E, size=k, replace=False)); c.append(np.full(k, col)); b.append(np.full(k, h))
    r, c, b = np.concatenate(r), np.concatenate(c), np.concatenate(b)
    ref = sparse.coo_matrix(((1 << b).astype(np.int64), (r, c)), shape=(E, T)).tocsr()
    ref.sort_indices()
    cps, cis = [], []
    for h in range(H):
        sel = b == h
        mh = sparse.coo_matrix((np.ones(int(sel.sum()), np.int8), (r[sel], c[sel])), shape=(E, T)).tocsc()
        mh.sort_indices()
        cps.append(mh.indptr.astype(np.int32)); cis.append(mh.indices.astype(np.int32))
    cp, ci = np.stack(cps), np.concatenate(cis)
    assert int(cp[:, 1].sum()) == n_col and int((cp[:, 2] - cp[:, 1]).sum()) == n_col
    want = (ref.indptr, ref.indices, ref.data.astype(np.int32))
    got = ecb.hapcsc_to_csr(torch.from_numpy(cp).cuda(), torch.from_numpy(ci).cuda(), E)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    for g, w in zip(ecb.hapcsc_to_csr_host(cp, ci, E), want):
        assert np.array_equal(g, w)
    ip, ix, da = (np.ascontiguousarray(x, dtype=np.int32) for x in want)
    dcp, dci = ecb.csr_to_hapcsc(*(torch.from_numpy(x).cuda() for x in (ip, ix, da)), T, H)
    assert np.array_equal(dcp.cpu().numpy(), cp) and np.array_equal(dci.cpu().numpy(), ci)
    hcp, hci = ecb.csr_to_hapcsc_host(ip, ix, da, T, H)
    assert np.array_equal(hcp, cp) and np.array_equal(hci, ci)
