"""``ecb_collapse_umis`` / ``ecb_collapse_umis_device`` (``--collapse-umis``) against the rule as ``tests/umi_checker.py`` states it:
every output compared exactly.  The sizes sit on the spans the kernels, the sort and the scan work in -- L records per lane, W per wave,
G per workgroup, TILE pairs per sort tile, STRETCH values per scan stretch, pinned to the source by ``tests/test_umi_constants.py``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from alntools_amd import ecb, ecb_umi as eu

import umi_checker as uc
from test_umi_constants import G, L, STRETCH, TILE, W

pytestmark = pytest.mark.gpu
PASS, FAIL = 0x0, 0x4
NONE32 = 0xFFFFFFFF
UMI_NONE = uc.UMI_NONE
N_LOCI, N_HAPS = 40, 4
MAX_LOCI = (1 << 26) - 3                 # the largest n_loci ecb_config allows


def build(reads, first_id=0, lead=0):
    """A stream from ``reads`` = lists of ``(passes, locus, haplotype)`` records, each beginning with a passing record (where the id
    steps); the first read's id is ``first_id``; ``lead`` non-passing records, carrying ``first_id - 1``, open the stream."""
    rid, loc, hf = [(first_id - 1) % (1 << 32)] * lead, [NONE32] * lead, [FAIL | 0xFFFF0000] * lead
    for k, read in enumerate(reads):
        assert read[0][0]
        for ok, l, h in read:
            rid.append((first_id + k) % (1 << 32))
            loc.append(l if ok else NONE32)                  # (nothing but the id is looked at in a record that does not pass)
            hf.append((h << 16) | PASS if ok else FAIL | 0xFF000000 | (h << 16))
    return np.array(rid, dtype=np.uint32), np.array(loc, dtype=np.uint32), np.array(hf, dtype=np.uint32)


def same(got, want):
    for k, name in enumerate(("read_id", "locus", "hapflag", "first_read")):
        g = got[k].cpu().numpy().view(np.uint32) if hasattr(got[k], "cpu") else got[k]
        assert len(g) == len(want[k]), "%s: %d entries, want %d (counts %r, want %r)" % (name, len(g), len(want[k]), got[4], want[4])
        bad = np.flatnonzero(g != want[k])
        assert len(bad) == 0, "%s[%d] of %d: %#x, want %#x" % (name, bad[0], len(g), g[bad[0]], want[k][bad[0]])
    assert got[4] == want[4]


def agree(rid, loc, hf, keys, n_loci=N_LOCI, n_haps=N_HAPS):
    keys = np.asarray(keys, dtype=np.uint64)
    assert uc.breach(rid, loc, hf, len(keys), n_loci, n_haps) is None
    want = uc.collapse(rid, loc, hf, keys)
    got = eu.collapse_umis(rid, loc, hf, keys, n_loci, n_haps)
    same(got, want)
    return got


def random_read(rng, base=None, p_fail=0.25, max_len=4):
    """A read of 1 .. max_len records; with ``base`` (a list of targets) it names most of those, so that intersections survive."""
    n = int(rng.integers(1, max_len + 1))
    rec = []
    for k in range(n):
        ok = k == 0 or rng.random() >= p_fail
        if base is not None and rng.random() < 0.8:
            l, h = base[int(rng.integers(len(base)))]
        else:
            l, h = int(rng.integers(N_LOCI)), int(rng.integers(N_HAPS))
        rec.append((ok, l, h))
    return rec


def molecule_stream(rng, sizes, order="adjacent"):
    """Molecules of the given sizes, each around a few targets of its own.  ``order``: ``adjacent`` -- a molecule's reads side by side;
    ``alternating`` -- the reads of molecules 2k and 2k + 1 interleaved; ``shuffled`` -- anywhere."""
    reads, keys = [], []
    for m, k in enumerate(sizes):
        base = [(int(rng.integers(N_LOCI)), int(rng.integers(N_HAPS))) for _ in range(int(rng.integers(1, 4)))]
        for _ in range(k):
            reads.append(random_read(rng, base))
            keys.append(1000 + m)
    idx = list(range(len(reads)))
    if order == "alternating":
        starts = np.concatenate(([0], np.cumsum(sizes)))
        idx = []
        for m in range(0, len(sizes), 2):
            a = list(range(starts[m], starts[m + 1]))
            b = list(range(starts[m + 1], starts[m + 2])) if m + 1 < len(sizes) else []
            for q in range(max(len(a), len(b))):
                idx += a[q:q + 1] + b[q:q + 1]
    elif order == "shuffled":
        idx = rng.permutation(len(reads)).tolist()
    return [reads[i] for i in idx], [keys[i] for i in idx]


def test_tiny_streams():
    rng = np.random.default_rng(1)
    for n_reads in range(1, L + 4):
        for _ in range(8):
            reads = [[(True, int(rng.integers(3)), int(rng.integers(2)))] for _ in range(n_reads)]
            keys = rng.integers(0, 2, size=n_reads)
            agree(*build(reads), keys)
            agree(*build(reads, first_id=7, lead=1), keys)
    # one record; a stream that holds no read at all
    got = agree(*build([[(True, 3, 1)]]), [5])
    assert got[0].tolist() == [0] and got[1].tolist() == [3] and got[2].tolist() == [1 << 16] and got[3].tolist() == [0] and got[4] == (1, 1, 0, 0, 1, 0)
    got = agree(np.array([9, 9], np.uint32), np.array([NONE32] * 2, np.uint32), np.array([FAIL] * 2, np.uint32), [])
    assert got[4] == (0,) * 6 and all(len(a) == 0 for a in got[:4])


@pytest.mark.parametrize("order", ["adjacent", "alternating", "ends"])
@pytest.mark.parametrize("k", [1, 2, 3, W + 1, 2 * G + 1, 300])
def test_molecule_sizes(k, order):
    rng = np.random.default_rng(k)
    if order == "ends":                                     # the molecule's reads at the two ends of the stream, others between
        reads, keys = molecule_stream(rng, [k] + [1, 2, 3] * 30)
        cut = (k + 1) // 2
        reads, keys = reads[:cut] + reads[k:] + reads[cut:k], keys[:cut] + keys[k:] + keys[cut:k]
    else:
        reads, keys = molecule_stream(rng, [2, k, k, 1, 3, k], order)
    got = agree(*build(reads), keys)
    assert got[4][2] >= (1 if k > 1 else 0)
    # ... and with one target that every read of the molecule names, so that it survives whatever else they say
    reads = [r + [(True, N_LOCI - 1, N_HAPS - 1)] for r in reads]
    got = agree(*build(reads), keys)
    assert got[4][3] == 0


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_edges(shift):
    """Reads of one record each, so that a read's index is its record's: a molecule's two (three) reads on either side of every wave,
    workgroup, sort-tile and scan-stretch edge -- in the stream, in the sorted keys (which ascend with the read) and, the other reads being
    molecules of two as well, in the sorted (molecule, target) pairs."""
    rng = np.random.default_rng(40 + shift)
    n = STRETCH + TILE + G + 3
    # pairs all over: reads 2j + shift, 2j + shift + 1 are molecule j
    mol = (np.arange(n) + 2 - shift) // 2
    for b in (W, G, TILE, STRETCH, STRETCH + TILE):
        lo = b + shift - 2
        mol[lo:lo + 3] = mol[lo]                            # a molecule of three (or four) over the edge
    loc = rng.integers(0, 3, size=n)
    hap = rng.integers(0, 2, size=n)
    reads = [[(True, int(loc[i]), int(hap[i]))] for i in range(n)]
    got = agree(*build(reads), mol.astype(np.uint64) * 3)
    assert got[4][3] > n // 8 and got[4][2] - got[4][3] > n // 16
    # singletons all over, one pair across each edge: the first sort's run heads at the edges, nothing else in the second sort
    keys = np.arange(n, dtype=np.uint64) * 2 + 10
    for b in (W, G, TILE, STRETCH):
        keys[b + shift - 1] = keys[b + shift - 2]
    got = agree(*build(reads), keys)
    assert got[4][2] == 4


def test_two_records_per_read_put_the_pairs_on_the_edges():
    """As above with reads of two and three records: the compacted pairs and their runs no longer line up with the reads."""
    rng = np.random.default_rng(50)
    reads, keys = [], []
    for m in range((STRETCH + G) // 5 + 1):
        t = (int(rng.integers(3)), int(rng.integers(2)))
        reads += [[(True,) + t, (rng.random() < 0.7, int(rng.integers(3)), 0)], [(True, int(rng.integers(3)), 1), (False, 0, 0), (True,) + t]]
        keys += [m, m]
    got = agree(*build(reads), keys)
    assert got[4][3] == 0 and got[4][4] >= len(reads) // 2


def test_one_molecule_of_every_read_and_every_read_its_own():
    rng = np.random.default_rng(6)
    reads = [random_read(rng, [(1, 0), (2, 1), (3, 1)]) + [(True, 7, 2)] for _ in range(2 * G + 37)]
    n = len(reads)
    got = agree(*build(reads), [77] * n)
    assert got[4][:5] == (n, 1, 1, 0, len(got[0])) and got[3].tolist() == [0] and (7, 2 << 16) in zip(got[1].tolist(), got[2].tolist())
    got = agree(*build(reads), np.arange(n)[::-1] * 5)       # distinct keys, falling: the numbering is the reads', not the keys'
    assert got[4][1:4] == (n, 0, 0) and got[3].tolist() == list(range(n))
    got = agree(*build(reads), [UMI_NONE] * n)
    assert got[4][1:4] == (n, 0, 0) and got[4][5] == n and got[3].tolist() == list(range(n))
    stream = build(reads)
    passing = np.array([uc.passes(int(h)) for h in stream[2]])
    assert np.array_equal(got[1], stream[1][passing]) and np.array_equal(got[2], stream[2][passing])      # as they are, in stream order


def test_extreme_keys_and_keys_equal_in_one_half_only():
    hi, lo = 5 << 32, 9
    keys = [0, UMI_NONE - 1, hi | lo, hi | (lo + 1), (hi + (1 << 32)) | lo, 0, UMI_NONE, UMI_NONE - 1, hi | lo, UMI_NONE, lo, hi, 1 << 63, (1 << 63) | lo, 1 << 63]
    reads = [[(True, 1, 0), (True, 2, 1)] for _ in keys]
    got = agree(*build(reads), keys)
    assert got[4] == (15, 11, 4, 0, 22, 2)
    assert got[3].tolist() == [0, 1, 2, 3, 4, 6, 9, 10, 11, 12, 13]


def test_a_duplicate_target_in_every_position_of_a_molecule():
    a, b, c = (True, 4, 1), (True, 9, 0), (True, 4, 2)
    for k in (2, 3):
        for who in range(k):                                 # read `who` names a twice, at positions p < q; another read lacks it or not
            for p in range(3):
                for q in range(p + 1, 4):
                    for lacking in (None,) + tuple(r for r in range(k) if r != who):
                        reads = []
                        for r in range(k):
                            rec = [b, c] if r == lacking else [a, b, c]
                            if r == who:
                                rec = [b, c]
                                rec.insert(p, a)
                                rec.insert(q, a)
                            reads.append(rec)
                        got = agree(*build([[(True, 0, 0)]] + reads + [[(True, 0, 0)]]), [1] + [2] * k + [3])
                        assert got[4][4] == 2 + (2 if lacking is not None else 3)
    # a singleton's duplicates stay
    got = agree(*build([[a, a, b, a]]), [UMI_NONE])
    assert got[1].tolist() == [4, 4, 9, 4] and got[0].tolist() == [0] * 4


def test_discarded_molecules():
    x, y = [(True, 1, 0)], [(True, 1, 1)]
    got = agree(*build([x, y, x, y, x, y]), [1, 1, 2, 2, 3, 3])           # every molecule discarded
    assert got[4] == (6, 3, 3, 3, 0, 0) and all(len(g) == 0 for g in got[:4])
    got = agree(*build([x, y, x, x, y]), [1, 1, 2, 2, 3])                 # the first one discarded: numbering starts at the second
    assert got[3].tolist() == [2, 4] and got[0].tolist() == [0, 1]
    got = agree(*build([x, x, y, x, y]), [1, 2, 1, 2, UMI_NONE])          # the first read's molecule discarded, the second's not
    assert got[3].tolist() == [1, 4]


def test_records_that_do_not_pass_in_front_inside_and_behind():
    reads = [[(True, 1, 0), (False, 2, 0), (True, 2, 1), (False, 1, 0)], [(True, 2, 1), (False, 1, 0), (True, 1, 0)], [(True, 5, 0), (False, 5, 1)],
             [(True, 1, 0), (False, 3, 3)]]
    for first_id, lead in ((0, 0), (0, 3), (0, W + 1), (5, 2), ((1 << 32) - 2, 0), ((1 << 32) - 2, 4)):
        got = agree(*build(reads, first_id, lead), [8, 8, 9, UMI_NONE])
        assert got[0].tolist() == [0, 0, 1, 2] and got[1].tolist() == [1, 2, 5, 1] and got[2].tolist() == [0, 1 << 16, 0, 0] and got[3].tolist() == [0, 2, 3]
    # a stream that opens with non-passing records carrying the first read's own id (no step): they are that read's
    rid, loc, hf = build(reads)
    agree(np.concatenate(([0, 0], rid)).astype(np.uint32), np.concatenate(([NONE32] * 2, loc)).astype(np.uint32),
          np.concatenate(([FAIL] * 2, hf)).astype(np.uint32), [8, 8, 9, UMI_NONE])
    # each term of the filter, with garbage in what does not pass
    rejected = [0x4, 0x1, 0x1 | 0x2 | 0x80, 0x1 | 0x2 | 0x1000, 0x1 | 0x2 | 0x2000]
    passing = [0x0, 0x1 | 0x2, 0x1000, 0x2000, 0x80, 0x10 | (3 << 16), 0x8000 | (1 << 16)]
    rid, loc, hf, keys = [], [], [], []
    for r, good in enumerate(passing):
        for bad in rejected:
            rid += [len(keys)] * 3
            loc += [r, NONE32, r + 1]
            hf += [good, bad | 0xFFFF0000, good]
            keys.append(r // 2 if bad & 0x1 else UMI_NONE)
    u32 = lambda a: np.array(a, dtype=np.uint32)
    agree(u32(rid), u32(loc), u32(hf), keys)


def test_the_largest_locus_and_haplotype():
    top = MAX_LOCI - 1
    reads = [[(True, top, 30), (True, 0, 30), (True, top, 0)], [(True, top, 0), (True, top, 30)], [(True, top, 30)], [(True, 0, 0), (True, top, 29)]]
    got = agree(*build(reads), [4, 4, 4, 4], n_loci=MAX_LOCI, n_haps=31)
    assert got[4][3] == 1
    got = agree(*build(reads[:3] + reads[:1]), [4, 4, 4, 9], n_loci=MAX_LOCI, n_haps=31)
    assert got[1].tolist() == [top, top, 0, top] and got[2].tolist() == [30 << 16, 30 << 16, 30 << 16, 0]
    # the other end -- one locus, one haplotype: the key is the molecule's rank alone -- and ranges that are no power of two
    one = [[(True, 0, 0)], [(True, 0, 0), (False, 0, 0), (True, 0, 0)], [(True, 0, 0)], [(True, 0, 0)], [(True, 0, 0)]]
    got = agree(*build(one), [1, 2, 1, 2, 2], n_loci=1, n_haps=1)
    assert got[4] == (5, 2, 2, 0, 2, 0) and got[1].tolist() == [0, 0] and got[2].tolist() == [0, 0]
    odd = [[(True, 4, 2), (True, 2, 0)], [(True, 2, 0), (True, 4, 2), (True, 3, 2)], [(True, 4, 1)]]
    got = agree(*build(odd), [6, 6, 7], n_loci=5, n_haps=3)
    assert got[1].tolist() == [2, 4, 4] and got[2].tolist() == [0, 2 << 16, 1 << 16]


def zipf_stream(seed, n=200000):
    """Some ``n`` records: reads of 1 .. 3 records, molecule sizes Zipf-distributed, a molecule's reads anywhere in the stream."""
    rng = np.random.default_rng(seed)
    n_reads = n // 2
    sizes = np.minimum(rng.zipf(2.2, size=n_reads), 4000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), n_reads)) + 1]
    mol = np.repeat(np.arange(len(sizes)), sizes)[:n_reads]
    mol = mol[rng.permutation(n_reads)]
    base = rng.integers(0, N_LOCI * N_HAPS, size=(len(sizes), 2))
    lens = rng.integers(1, 4, size=n_reads)
    rid = np.repeat(np.arange(n_reads), lens)
    head = np.concatenate(([True], rid[1:] != rid[:-1]))
    m = len(rid)
    own = rng.random(m) < 0.15
    target = np.where(own, rng.integers(0, N_LOCI * N_HAPS, size=m), base[mol[rid], rng.integers(0, 2, size=m)])
    ok = (rng.random(m) >= 0.15) | head
    hf = np.where(ok, PASS, FAIL).astype(np.uint32) | ((target % N_HAPS) << 16).astype(np.uint32)
    keys = np.where(rng.random(n_reads) < 0.05, UMI_NONE, (mol.astype(np.uint64) << np.uint64(33)) | np.uint64(1 << 32)).astype(np.uint64)
    return rid.astype(np.uint32), (target // N_HAPS).astype(np.uint32), hf, keys


_ZIPF = {}


def _zipf():
    if not _ZIPF:
        s = zipf_stream(11)
        _ZIPF["s"] = (s, uc.collapse(*s))
    return _ZIPF["s"]


def test_a_random_stream_with_zipf_molecule_sizes():
    s, want = _zipf()
    assert uc.breach(s[0], s[1], s[2], len(s[3]), N_LOCI, N_HAPS) is None
    same(eu.collapse_umis(*s, N_LOCI, N_HAPS), want)
    c = want[4]
    assert c[2] > 5000 and c[3] > 500 and c[2] - c[3] > 500 and c[5] > 1000 and np.bincount((s[3][s[3] != UMI_NONE] >> np.uint64(33)).astype(np.int64)).max() > 1000


def test_one_rule_for_every_route(monkeypatch):
    import torch
    s, want = _zipf()
    first = eu.collapse_umis(*s, N_LOCI, N_HAPS)
    again = eu.collapse_umis(*s, N_LOCI, N_HAPS)
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in s[:3]] + [torch.from_numpy(s[3].view(np.int64)).cuda()]
    tens = eu.collapse_umis(*dev, N_LOCI, N_HAPS)
    tens2 = eu.collapse_umis(*dev, N_LOCI, N_HAPS)
    monkeypatch.setenv("ECB_POISON_SCRATCH", "1")
    poisoned = [eu.collapse_umis(*s, N_LOCI, N_HAPS), eu.collapse_umis(*dev, N_LOCI, N_HAPS), eu.collapse_umis(*s, N_LOCI, N_HAPS)]
    monkeypatch.delenv("ECB_POISON_SCRATCH")
    for got in [first, again, tens, tens2] + poisoned:
        same(got, want)
    assert tens[0].is_cuda and tens[3].is_cuda


def test_the_output_is_a_stream_the_handle_takes_with_cells_from_first_read():
    from oracle import ec_oracle as orc
    s, want = _zipf()
    rng = np.random.default_rng(5)
    n_reads = len(s[3])
    meta = (rng.integers(0, 50, size=n_reads) | (rng.integers(0, 3, size=n_reads) << 22)).astype(np.uint32)
    rid, loc, hf, first, counts = eu.collapse_umis(*s, N_LOCI, N_HAPS)
    with ecb.EcBuilder(N_LOCI, N_HAPS, multisample=True) as b:
        b.push(rid, loc, hf)
        b.push_cells(meta[first], 0)
        sizes = b.finalize()
        a = b.export()
        pairs = b.export_pairs()
    ref = orc.ec_from_tuples(want[0], want[1], want[2], N_LOCI, N_HAPS)
    assert sizes["n_reads"] == len(want[3]) == counts[1] - counts[3] and sizes["valid_alignments"] == sizes["all_alignments"] == counts[4]
    assert np.array_equal(a["indptrA"], ref["indptr"]) and np.array_equal(a["indicesA"], ref["indices"]) and np.array_equal(a["dataA"], ref["data"])
    # the triples: every molecule counts once, in the cell and the file of its first read
    ec_of, per = {}, {}
    start = np.flatnonzero(np.concatenate(([True], want[0][1:] != want[0][:-1], [True])))
    for m in range(len(want[3])):
        key = tuple(sorted({(int(want[1][i]), int(want[2][i]) >> 16) for i in range(start[m], start[m + 1])}))
        e = ec_of.setdefault(key, len(ec_of))
        mt = int(meta[want[3][m]])
        t = (e, mt & ((1 << 22) - 1), mt >> 22)
        per.setdefault(t, [0, m])[0] += 1
    trip = sorted(per)
    assert pairs["ec"].tolist() == [t[0] for t in trip] and pairs["cell"].tolist() == [t[1] for t in trip] and pairs["file"].tolist() == [t[2] for t in trip]
    assert pairs["count"].tolist() == [per[t][0] for t in trip] and pairs["first"].tolist() == [per[t][1] for t in trip]
    assert int(ref["count"].sum()) == len(want[3]) and np.array_equal(np.bincount(pairs["ec"], weights=pairs["count"]).astype(np.int64), ref["count"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw(rid, loc, hf, keys, n=None, n_reads=None, n_loci=N_LOCI, n_haps=N_HAPS, outs=None, counts=True, skip=None):
    lib = eu.load()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n = len(rid) if n is None else n
    outs = [np.full(max(len(rid), 1), 0x5C5C5C5C, dtype=np.uint32) for _ in range(4)] if outs is None else outs
    cnt = (C.c_uint64 * 6)(*[7] * 6)
    P = ecb._ptr
    ptrs = [P(rid), P(loc), P(hf), P(keys)] + [P(o) for o in outs]
    if skip is not None:
        ptrs[skip] = None
    rc = lib.ecb_collapse_umis(0, ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, len(keys) if n_reads is None else n_reads, n_loci, n_haps, ptrs[4], ptrs[5],
                               ptrs[6], ptrs[7], cnt if counts else None)
    untouched = all((o == 0x5C5C5C5C).all() for o in outs) and tuple(cnt) == (7,) * 6
    return rc, (lib.ecb_last_error(None) or b"").decode(), untouched


def _short_reads(rng, n):
    head = rng.random(n) < 0.4
    head[0] = True
    ok = (rng.random(n) >= 0.2) | head
    rid = (np.cumsum(head) - 1).astype(np.uint32)
    keys = rng.integers(0, max(int(rid[-1]) // 2, 1), size=int(rid[-1]) + 1).astype(np.uint64)
    return rid, rng.integers(0, N_LOCI, size=n).astype(np.uint32), (np.where(ok, PASS, FAIL) | (rng.integers(0, N_HAPS, size=n) << 16)).astype(np.uint32), keys


def test_refused_arguments_write_nothing():
    rng = np.random.default_rng(3)
    s = _short_reads(rng, 50)
    for kw in (dict(n=0), dict(n_haps=0), dict(n_haps=32), dict(n_loci=0), dict(n_loci=MAX_LOCI + 1), dict(counts=False)) + tuple(dict(skip=k) for k in range(8)):
        r = _raw(*s, **kw)
        assert r[0] == -1 and r[1].startswith("umi: ") and r[2], (kw, r)
    r = _raw(*s, n=1 << 30)
    assert r[0] == -8 and "2^30" in r[1] and r[2]
    assert _raw(*s, n_loci=MAX_LOCI, n_haps=31)[0] == 0
    # an output that shares a byte with an input or with another output
    lib, P = eu.load(), ecb._ptr
    big = np.zeros(400, dtype=np.uint32)
    big[:50], big[100:150], big[200:250] = s[0], s[1], s[2]
    key_words = s[3].view(np.uint32)
    o = [np.zeros(50, np.uint32) for _ in range(4)]
    cnt = (C.c_uint64 * 6)()
    for outs in ((big[49:99], o[1], o[2], o[3]), (o[0], big[100:150], o[2], o[3]), (o[0], o[1], big[249:299], o[3]), (o[0], o[1], o[2], big[0:50]),
                 (o[0], o[0], o[2], o[3]), (o[0], o[1], o[2], o[2][1:]), (o[0], o[1], o[2], key_words), (big[0:50], o[1], o[2], o[3])):
        before = big.copy()
        rc = lib.ecb_collapse_umis(0, P(big[0:50]), P(big[100:150]), P(big[200:250]), P(s[3]), 50, len(s[3]), N_LOCI, N_HAPS, *[P(x) for x in outs], cnt)
        assert rc == -1 and b"overlaps" in lib.ecb_last_error(None) and np.array_equal(big, before)
    assert lib.ecb_collapse_umis(0, P(big[0:50]), P(big[100:150]), P(big[200:250]), P(s[3]), 50, len(s[3]), N_LOCI, N_HAPS, *[P(x) for x in o], cnt) == 0
    assert tuple(cnt) == uc.collapse(*s)[4]


@pytest.mark.parametrize("at", [1, W - 1, W, G, 2 * G + 1, 2 * G + W + 3])
def test_a_broken_contract_names_the_lowest_offender_and_writes_nothing(at):
    rng = np.random.default_rng(at)
    n = 2 * G + W + 5
    for reason in ("read_id falls", "read_id steps by more than 1", "read_id steps on a record that does not pass the filter", "locus at or beyond n_loci",
                   "haplotype at or beyond n_haps"):
        rid, loc, hf, keys = _short_reads(rng, n)
        if reason == "read_id falls":
            rid[at:] -= np.uint32(rid[at] - rid[at - 1] + 1)
        elif reason == "read_id steps by more than 1":
            rid[at:] += np.uint32(2)
        elif reason.startswith("read_id steps on"):
            rid[at:] += np.uint32(1 - (rid[at] - rid[at - 1]))
            hf[at] = FAIL
        elif reason.startswith("locus"):
            hf[at] &= np.uint32(0xFFFF0000)
            loc[at] = N_LOCI
        else:
            hf[at] = N_HAPS << 16 if at % 2 else 1 << 24           # (a bit among 24 .. 31 is a haplotype beyond any n_haps)
        if at + 300 < n:                                           # a second, higher offender: the lowest is named
            rid[at + 300:] += np.uint32(5)
        assert uc.breach(rid, loc, hf, len(keys), N_LOCI, N_HAPS) == (at, reason)
        rc, msg, untouched = _raw(rid, loc, hf, keys)
        assert rc == ecb.ECB_ERR_CONTRACT and msg == "umi: record %d: %s" % (at, reason) and untouched, msg
        with pytest.raises(eu.UmiContractError) as e:
            eu.collapse_umis(rid, loc, hf, keys, N_LOCI, N_HAPS)
        assert e.value.record == at
    # ids that make no sense at all address nothing outside the buffers: the call is refused, and the next one is right
    rid, loc, hf, keys = _short_reads(rng, n)
    rc, msg, untouched = _raw(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32), loc, hf, keys)
    assert rc == ecb.ECB_ERR_CONTRACT and untouched
    agree(rid, loc, hf, keys)


@pytest.mark.parametrize("lead", [0, 3])
def test_an_n_reads_that_is_not_the_streams(lead):
    rng = np.random.default_rng(9)
    reads = [random_read(rng) for _ in range(G + 9)]
    rid, loc, hf = build(reads, first_id=4, lead=lead)
    starts = np.flatnonzero(np.concatenate(([lead == 0], rid[1:] != rid[:-1])))
    assert len(starts) == len(reads)
    for n_reads in (0, 1, W, len(reads) - 1, len(reads) + 1, 3 * len(reads), 1 << 40):
        keys = np.zeros(min(n_reads, 4 * len(reads)) + 1, np.uint64)
        at = int(starts[n_reads]) if n_reads < len(reads) else len(rid) - 1
        want = (at, "the stream holds %d reads, n_reads is %d" % (len(reads), n_reads))
        assert n_reads > len(keys) or uc.breach(rid, loc, hf, n_reads, N_LOCI, N_HAPS) == want
        rc, msg, untouched = _raw(rid, loc, hf, keys, n_reads=n_reads)
        assert rc == ecb.ECB_ERR_CONTRACT and msg == "umi: record %d: %s" % want and untouched, msg
    # a stream without a passing record holds no read: one key is one too many
    rc, msg, untouched = _raw(np.zeros(5, np.uint32), np.zeros(5, np.uint32), np.full(5, FAIL, np.uint32), np.zeros(1, np.uint64))
    assert rc == ecb.ECB_ERR_CONTRACT and msg == "umi: record 4: the stream holds 0 reads, n_reads is 1" and untouched


# ---- end to end through the command line --------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g4b_gen():
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import g4b_gen
    return g4b_gen


def _qname(g4b_gen, read, cell, umi):
    f = g4b_gen._qname(read, cell).split("|||")
    f[6] = umi
    return "|||".join(f)


def _umi_files(seed, n_files=3, reads=220, with_scores=False):
    """Seeded reads in the manner of ``tests/golden/g4b_gen.py`` (its references, its names -- without a space: with the reference's
    untrimmed-name quirk every record of a spaced name is a run of its own), each with a seeded ACGT UMI in field 6.  About a third of
    the reads share a molecule -- same cell, same UMI -- with another read, some of them across files; some molecules' reads share no
    target.  Every file ends in one extra read, which the reference's rule drops.
    -> per file a list of reads ``(name, cell, umi, [(flag, tid, pos, NM)])``, the last one the extra read."""
    g4b_gen = _g4b_gen()
    rng = np.random.RandomState(seed)
    n = n_files * reads
    umis = ["".join("ACGT"[int(x)] for x in rng.randint(4, size=10)) for _ in range(n)]
    cells = ["BC%04d" % rng.randint(6) for _ in range(n)]
    genes = [int(rng.randint(g4b_gen.N_GENES)) for _ in range(n)]
    for i in range(n):                                       # a third of the reads take the cell, the UMI and mostly the gene of an earlier one
        if i and rng.rand() < 0.2:
            j = int(rng.randint(i)) if rng.rand() < 0.5 else max(i - 1 - int(rng.randint(5)), 0)
            umis[i], cells[i] = umis[j], cells[j]
            if rng.rand() < 0.8:
                genes[i] = genes[j]
    files = []
    for fi in range(n_files):
        out = []
        for r in range(reads + 1):
            i = fi * reads + r
            last = r == reads
            umi, cell, g = ("ACGT", "BC0000", 0) if last else (umis[i], cells[i], genes[i])
            if not last and rng.rand() < 0.04:
                umi = ["", "ACGN", "acgt", "A" * 17][int(rng.randint(4))]             # no UMI: a molecule of its own
            name = _qname(g4b_gen, "f%dr%05d" % (fi, r), cell, umi)
            tids = [2 * g, 2 * g + 1] if rng.rand() < 0.7 else [2 * g + int(rng.randint(2))]
            if rng.rand() < 0.3:
                g2 = (g + 1 + int(rng.randint(3))) % g4b_gen.N_GENES
                tids += [2 * g2, 2 * g2 + 1]
            if rng.rand() < 0.15:
                tids.append(tids[0])                                                   # a target named twice
            recs = [(16 if rng.rand() < 0.5 else 0, int(t), int(rng.randint(500)), int(rng.randint(3))) for t in tids]
            if rng.rand() < 0.1:
                recs.insert(int(rng.randint(len(recs))) + 1, (4, -1, -1, 0))          # an unmapped record inside the read
            out.append((name, cell, umi, recs))
        files.append(out)
    return files


def _write(path, refs, reads, with_tags):
    from alntools_amd import bamio
    recs = [(name, flag, tid, pos, -1, -1) for name, _, _, rr in reads for flag, tid, pos, _ in rr]
    tags = [[("NM", "C", nm)] for _, _, _, rr in reads for _, _, _, nm in rr] if with_tags else None
    bamio.write_bam(path, refs, recs, tags=tags)


def _collapsed_files(files, refs, strata):
    """The second directory: the checker's rule over the counted reads of all files (after best-strata on NM where ``strata``); every
    surviving molecule one read at its first read's place, every file's extra read behind them."""
    rid, loc, hf, keys, where, cell_ids = [], [], [], [], [], {}
    for fi, reads in enumerate(files):
        for r, (name, cell, umi, recs) in enumerate(reads[:-1]):
            if strata:
                best = min(nm for flag, _, _, nm in recs if uc.passes(flag))
                recs = [x for x in recs if uc.passes(x[0]) and x[3] == best]     # (what does not pass names nothing)
            for flag, tid, pos, nm in recs:
                rid.append(len(keys))
                loc.append(max(tid, 0) // 2)                  # (g4b's targets: gene g has the references 2g and 2g + 1, its two haplotypes)
                hf.append(flag | ((max(tid, 0) % 2) << 16))
            code = eu.pack_umi(umi)
            keys.append(UMI_NONE if code is None else (cell_ids.setdefault(cell, len(cell_ids)) << 33) | code)
            cell_ids.setdefault(cell, len(cell_ids))
            where.append((fi, r))
    u32 = lambda a: np.array(a, dtype=np.uint32)
    out_id, out_loc, out_hf, first, counts = uc.collapse(u32(rid), u32(loc), u32(hf), np.array(keys, dtype=np.uint64))
    assert counts[2] > 30 and counts[3] > 3 and counts[5] > 5 and counts[2] - counts[3] > 20
    second = [[] for _ in files]
    start = np.flatnonzero(np.concatenate(([True], out_id[1:] != out_id[:-1], [True])))
    for m, f in enumerate(first):
        fi, r = where[int(f)]
        name, cell, umi, _ = files[fi][r]
        recs = [(0, 2 * int(out_loc[i]) + (int(out_hf[i]) >> 16), 10, 0) for i in range(start[m], start[m + 1])]
        second[fi].append((name, cell, umi, recs))
    for fi, reads in enumerate(files):
        second[fi].append(reads[-1])
    crosses = sum(1 for k in set(keys) if k != UMI_NONE and len({where[i][0] for i, x in enumerate(keys) if x == k}) > 1)
    assert crosses > 5
    return second, counts


_E2E = {}


def _run(args):
    from click.testing import CliRunner
    from alntools_amd import cli, utils
    level = utils.get_logger().level
    try:
        r = CliRunner().invoke(cli.cli, args)
    finally:
        utils.get_logger().setLevel(level)                  # (the command sets the package's log level: later tests find it as it was)
    assert r.exit_code == 0, (args, r.output, r.exception)


@pytest.mark.parametrize("decoder", ["py", "c"])
@pytest.mark.parametrize("command", ["bam2ec", "bam2emase"])
def test_the_option_end_to_end(tmp_path, monkeypatch, command, decoder):
    """The directory with every read, run WITH the option, gives the bytes of the directory that holds one read per surviving molecule,
    run without it -- under ``-m -1`` and ``-m 40`` --; run without the option it does not."""
    monkeypatch.setenv("ALNTOOLS_DECODER", decoder)
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    g4b_gen = _g4b_gen()
    refs = g4b_gen.references()
    if "files" not in _E2E:
        _E2E["files"] = _umi_files(41)
        _E2E["second"] = _collapsed_files(_E2E["files"], refs, strata=False)[0]
    for kind in ("all", "second"):
        os.makedirs(str(tmp_path / kind))
        for fi, reads in enumerate(_E2E["files" if kind == "all" else "second"]):
            _write(str(tmp_path / kind / ("m_%d.bam" % fi)), refs, reads, with_tags=False)

    def run(kind, option, mincount):
        out = str(tmp_path / ("%s_%d_%d.out" % (kind, option, mincount)))
        _run([command, str(tmp_path / kind), out, "--multisample", "-m", str(mincount)] + (["--collapse-umis"] if option else []))
        if command == "bam2emase":
            _run(["emase2ec", out, out + ".bin"])
            out += ".bin"
        return out
    for mincount in (-1, 40):
        with_option, second, without = (open(run(*a, mincount), "rb").read() for a in (("all", 1), ("second", 0), ("all", 0)))
        assert with_option == second, "-m %d" % mincount
        assert without != with_option
    if command == "bam2ec":                                  # ecquant-cells runs on the result
        out = run("all", 1, -1)
        _run(["ecquant-cells", out, str(tmp_path / "cells.tsv")])
        assert os.path.getsize(str(tmp_path / "cells.tsv")) > 0


@pytest.mark.parametrize("decoder", ["py", "c"])
def test_names_without_a_umi_give_the_golden_bytes(tmp_path, monkeypatch, decoder):
    """The g4b names have ``x6`` in field 6, which is no UMI: every read is a molecule of its own, and the option changes nothing."""
    monkeypatch.setenv("ALNTOOLS_DECODER", decoder)
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    import json
    from alntools_amd import bamio
    g4b_gen = _g4b_gen()
    g = json.load(open(os.path.join(GOLDEN, "g4b_multi.json")))
    recs = g4b_gen.files(g["seed"])
    src = str(tmp_path / "g4b")
    os.makedirs(src)
    for k, fname in enumerate(g["glob_order"]):            # (the command sorts the names: numbered, they sort into the order the golden was made in)
        bamio.write_bam(os.path.join(src, "%02d_%s" % (k, fname)), g4b_gen.references(), recs[fname])
    for mincount in g4b_gen.MINCOUNTS:
        out = str(tmp_path / ("min%d.bin" % mincount))
        _run(["bam2ec", src, out, "--multisample", "-m", str(mincount), "--collapse-umis"])
        assert open(out, "rb").read() == open(os.path.join(GOLDEN, "g4b_multi_min%s.bin" % (mincount if mincount > 0 else "0")), "rb").read(), mincount


def test_best_strata_then_collapse(tmp_path, monkeypatch):
    monkeypatch.setenv("ALNTOOLS_DECODER", "c")
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    refs = _g4b_gen().references()
    files = _umi_files(43)
    second, counts = _collapsed_files(files, refs, strata=True)
    for kind, data in (("all", files), ("second", second)):
        os.makedirs(str(tmp_path / kind))
        for fi, reads in enumerate(data):
            _write(str(tmp_path / kind / ("m_%d.bam" % fi)), refs, reads, with_tags=True)
    outs = []
    for kind, opts in (("all", ["--best-strata", "NM", "--collapse-umis"]), ("second", []), ("all", ["--collapse-umis"])):
        out = str(tmp_path / ("%s_%d.bin" % (kind, len(opts))))
        _run(["bam2ec", str(tmp_path / kind), out, "--multisample", "-m", "-1"] + opts)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[2] != outs[0]
