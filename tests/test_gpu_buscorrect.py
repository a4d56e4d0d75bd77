"""Barcode correction on the GPU (``ecb_bus_correct`` / ``ecb_bus_correct_device``, ``bus2ec -w``, ``buscorrect``), every output -- records,
status, sizes -- compared exactly with the checker (``tests/bus_correct_checker.py``).  (1) BUS directories made from the golden ``.bin``
files with every fifth barcode one base off and 1 % more records two bases off must convert back to the golden bytes through the command
line with ``-w`` and must not without it; (2) every barcode length with an edge in it; (3) every number of candidates; (4) the directory's
and the buckets' edges (the constants come from ``test_bus_correct_constants.py``); (5) record, miss and kept counts around a workgroup, a
wave and a scan stretch; (6) one rule for every route; (7) every refusal; (8) ``ecquant-cells`` on the result.

All shapes stay at or below 33 000 records and a whitelist of about a million entries."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, bus_utils, ecb, ecb_bus, ecb_bus_correct as ebc

import bus_checker as bc
import bus_correct_checker as cc
from test_bus_correct_constants import BUSC_BISECT_LEN, BUSC_BUCKET_AVG, BUSC_LANES, SCB, TPB, dir_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARG, LIMIT, CONTRACT = -1, -8, -5             # include/ecb.h: ECB_ERR_ARG, ECB_ERR_LIMIT, ECB_ERR_CONTRACT
_kept = {}


def _np(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.asarray(x)


def _white(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.uint64)


def _rec(barcodes, seed=0):
    """Records of these barcodes whose other 24 bytes are all in use: the UMI, ec, count, flags and pad random."""
    n = len(barcodes)
    rng = np.random.default_rng(seed)
    rec = bc.records(np.array(barcodes, dtype=np.uint64), rng.integers(0, 1 << 63, size=n).astype(np.uint64), rng.integers(-5, 1 << 30, size=n),
                     rng.integers(0, 1 << 32, size=n), flags=rng.integers(0, 1 << 32, size=n))
    rec[:, 28:] = rng.integers(0, 256, size=(n, 4))
    return rec


def _library(rec, bclen, white, tensors=False, want_status=True):
    if tensors:
        import torch
        rec = torch.as_tensor(np.ascontiguousarray(rec), device="cuda")
    out, status, sizes = ebc.correct(rec, bclen, white, want_status=want_status)
    return _np(out), (None if status is None else _np(status)), sizes


def _exact(rec, bclen, white, tensors=False):
    """The library's three outputs against the checker's, exactly; -> the checker's (status, kept, sizes)."""
    want = cc.correct(rec, bclen, white)
    out, status, sizes = _library(rec, bclen, white, tensors)
    assert sizes == want[2], (sizes, want[2])
    assert status.dtype == np.uint8 and np.array_equal(status, want[0]), np.flatnonzero(status != want[0])[:10]
    assert out.dtype == np.uint8 and out.shape == want[1].shape and np.array_equal(out, want[1])
    return want


def _sub(seq, pos, step):
    """``seq`` with the base at ``pos`` moved ``step`` letters on in ACGT (step 1 .. 3: another base)."""
    return seq[:pos] + bc.BASES[(bc.BASES.index(seq[pos]) + step) % 4] + seq[pos + 1:]


# ---- 1. the golden files end to end ---------------------------------------------------------------------------------------------------------
def _cli_env():
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    return env


GOLD = {"g4b": ("g4b_multi_min0.bin", 3, {0: "g4b_multi_min0.bin", 40: "g4b_multi_min40.bin", 160: "g4b_multi_min160.bin"}),
        "g4": ("g4_multi_min0.bin", 6, {20: "g4_multi_min20.bin", 60: "g4_multi_min60.bin"})}
VARIANTS = {"plain": {}, "split-shuffled": dict(split=True, shuffle=True), "no-umi": dict(no_umi=True)}
PAIRS = [(p, q) for p in range(16) for q in range(p + 1, 16)]                # the fixed order in which two positions are tried


def _corrupted(m, path, variant, apart):
    """``bus_from_bin(seed=0)``'s directory with its barcodes damaged, and the whitelist that repairs it: -> (b, whitelist file, the
    records as damaged, the whitelist, the numbers of records changed in one base and added with two)."""
    b = bc.bus_from_bin(m, path, seed=0, **variant)
    cells = [bc.decode(v, 16) for v in b["values"]]
    key = ("whitelist", tuple(cells))                                         # (the seed decides the cells: one whitelist per golden file)
    if key not in _kept:
        assert min(cc.distance(x, y) for i, x in enumerate(cells) for y in cells[:i]) >= apart
        rng = np.random.default_rng(99)
        decoys = []
        while len(decoys) < 50:
            d = "".join(rng.choice(list(bc.BASES), size=16))
            if all(cc.distance(d, x) >= 3 for x in cells) and d not in decoys:
                decoys.append(d)
        white = _white([bc.encode(s) for s in cells + decoys])
        assert len(white) == len(cells) + 50
        listed = set(white.tolist())
        for v in b["values"].tolist():                                        # all 48 single-base changes of every cell come back to it
            assert all(cc.outcome(bc.encode(s), 16, listed) == (cc.CORRECTED, v) for s in cc.neighbours(bc.decode(v, 16)))
        _kept[key] = white
    white = _kept[key]
    wset = set(white.tolist())
    rec = b["records"].copy()
    r = rec.reshape(-1).view(cc._REC)
    n = len(r)
    one = np.arange(0, n, 5)
    for i in one.tolist():
        r["bc"][i] = bc.encode(_sub(bc.decode(r["bc"][i], 16), i % 16, 1 + i % 3))
    extra = r[np.arange(50, n, 100)].copy()
    for k in range(len(extra)):
        seq = bc.decode(extra["bc"][k], 16)
        for p, q in PAIRS:
            two = bc.encode(_sub(_sub(seq, p, 1 + k % 3), q, 1 + (k // 3) % 3))
            if cc.outcome(two, 16, wset)[0] == cc.NO_CANDIDATE:
                break
        else:
            raise AssertionError("no two-base change of %s is without a candidate" % seq)
        extra["bc"][k], extra["umi"][k] = two, (1 << 23) + k                  # (a UMI of its own)
    at = np.sort(np.random.default_rng(5).integers(0, n + 1, size=len(extra)))
    damaged = np.insert(r, at, extra).view(np.uint8).reshape(-1, 32)
    hdr = bus_utils.read_header(os.path.join(b["dir"], "output.bus"))
    with open(os.path.join(b["dir"], "output.bus"), "r+b") as fh:
        head = fh.read(hdr.offset)
        fh.seek(hdr.offset)
        fh.write(damaged.tobytes())
    wl = os.path.join(path, "whitelist.txt")
    order = np.random.default_rng(6).permutation(len(white))                  # (the file is not sorted)
    with open(wl, "w") as fh:
        fh.write("".join(bc.decode(white[j], 16) + "\n" for j in order))
    return b, wl, damaged, white, head, len(one), len(extra)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", list(GOLD))
def test_a_damaged_golden_directory_converts_back_byte_for_byte_with_the_whitelist(tmp_path, which, variant):
    source, apart, wants = GOLD[which]
    m = bin_utils.ecload(os.path.join(GOLDEN, source))
    b, wl, damaged, white, head, n_one, n_two = _corrupted(m, str(tmp_path / "bus"), VARIANTS[variant], apart)
    n = len(damaged)
    assert n_one == (n - n_two + 4) // 5 and n_two >= max((n - n_two) // 100, 1)
    status, kept, sizes = cc.correct(damaged, 16, white)
    assert sizes == (n - n_one - n_two, n_one, n_two, 0) and np.array_equal(kept, b["records"])
    more = ["--no-umi"] if variant == "no-umi" else []
    for k, (mincount, golden) in enumerate(sorted(wants.items())):
        out, stats = str(tmp_path / ("m%d.bin" % mincount)), str(tmp_path / ("m%d.stats" % mincount))
        argv = [b["dir"], out, "-w", wl, "-m", str(mincount), "--names", b["names"], "-l", b["lengths"], "--stats", stats] + more
        r = subprocess.run([sys.executable] + (["-X", "importtime"] if k == 0 else []) + ["-m", "alntools_amd.cli", "bus2ec"] + argv, cwd=ROOT,
                           env=_cli_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        if k == 0:
            imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
            assert "alntools_amd.ecb_bus_correct" in imported and not any(x == "torch" or x.startswith("torch.") for x in imported)
        with open(out, "rb") as got, open(os.path.join(GOLDEN, golden), "rb") as want:
            assert got.read() == want.read(), (which, variant, mincount)
        lines = dict(l.split("\t") for l in open(stats).read().splitlines())
        assert list(lines)[:7] == list(bus_utils.STATS) and list(lines)[7:] == list(bus_utils.WHITELIST_STATS)
        assert [int(lines[x]) for x in ("records",) + bus_utils.WHITELIST_STATS] == [n, n - n_one - n_two, n_one, n_two, 0]
    # the same directory without -w is another file
    mincount, golden = sorted(wants.items())[0]
    out = str(tmp_path / "without.bin")
    bus_utils.convert(b["dir"], out, no_umi=variant == "no-umi", mincount=mincount, names_file=b["names"], lengths_file=b["lengths"])
    with open(out, "rb") as got, open(os.path.join(GOLDEN, golden), "rb") as want:
        assert got.read() != want.read()
    # buscorrect: the header as it is, then the checker's records
    fixed, stats = str(tmp_path / "fixed.bus"), str(tmp_path / "fixed.stats")
    bus_utils.correct_file(os.path.join(b["dir"], "output.bus"), fixed, wl, stats_file=stats)
    with open(fixed, "rb") as fh:
        assert fh.read() == head + kept.tobytes()
    assert open(stats).read() == ("records\t%d\nbarcodes_exact\t%d\nbarcodes_corrected\t%d\nbarcodes_without_candidate\t%d\nbarcodes_ambiguous\t0\n"
                                  % (n, n - n_one - n_two, n_one, n_two))


def test_a_whitelist_next_to_no_record_is_refused_and_no_file_is_left(tmp_path):
    m = bin_utils.ecload(os.path.join(GOLDEN, "g4_multi_min0.bin"))
    b = bc.bus_from_bin(m, str(tmp_path / "bus"), seed=0)
    cells = set(b["values"].tolist())
    far = [s for s in ("ACGT" * 4, "TTTT" * 4, "GATC" * 4) if all(cc.outcome(v, 16, {bc.encode(s)})[0] == cc.NO_CANDIDATE for v in cells)]
    wl = str(tmp_path / "far.txt")
    with open(wl, "w") as fh:
        fh.write("\n".join(far) + "\n")
    assert far
    for argv, out in ((["bus2ec", b["dir"], str(tmp_path / "out.bin"), "-w", wl, "--stats", str(tmp_path / "s.txt")], "out.bin"),
                      (["buscorrect", os.path.join(b["dir"], "output.bus"), str(tmp_path / "out.bus"), "-w", wl], "out.bus")):
        r = subprocess.run([sys.executable, "-m", "alntools_amd.cli"] + argv, cwd=ROOT, env=_cli_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "Error: " in r.stderr and "output.bus: no record has a barcode on or next to the whitelist" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(str(tmp_path / out)) and not os.path.exists(str(tmp_path / "s.txt"))


# ---- 2. barcode lengths and bit edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bclen", [1, 2, 16, 21, 22, 31, 32])
def test_barcode_lengths_and_bit_edges(bclen):
    """3 x bclen neighbours: 63 (one round of a wave, one lane idle) at 21, 66 (two rounds) at 22, 96 at 32, where the first base sits in
    bits 62 and 63 and the mask of used bits is all ones."""
    assert BUSC_LANES == 64 and 3 * 21 == 63 and 3 * 22 == 66
    rng = np.random.default_rng(bclen)
    zero, ones = "A" * bclen, "T" * bclen
    some = ["".join(rng.choice(list(bc.BASES), size=bclen)) for _ in range(6)] if bclen > 2 else []
    places = sorted({0, bclen // 2, bclen - 1})

    def probes(seqs):
        return [s for s in seqs] + [_sub(s, p, step) for s in seqs for p in places for step in (1, 2, 3)] + \
               [_sub(_sub(s, places[0], 1), places[-1], 2) for s in seqs if bclen > 1]
    listed = [zero, ones] + some
    rec = _rec([bc.encode(s) for s in probes(listed + ["C" * bclen])], seed=bclen)
    want = _exact(rec, bclen, _white(bc.encode(s) for s in listed))
    assert want[2][0] >= len(listed) and (bclen <= 2 or want[2][1] >= 9 * len(listed) - 9) and (bclen <= 2 or want[2][2] > 0)
    if bclen == 32:
        assert any(int(v) >> 62 == 3 for v in bc.fields(want[1])[0]) and bc.encode(ones) == (1 << 64) - 1
    # a whitelist of one entry: barcode 0, then the all-ones barcode
    for only in (zero, ones):
        want = _exact(rec, bclen, _white([bc.encode(only)]))
        assert want[2][0] >= 1 and want[2][1] >= 3 * len(places) and want[2][3] == 0      # (one entry: never two candidates)
    if bclen <= 2:
        every = ["".join(t) for t in (bc.BASES if bclen == 1 else [x + y for x in bc.BASES for y in bc.BASES])]
        rec = _rec([bc.encode(s) for s in every] * 3, seed=1)
        want = _exact(rec, bclen, _white(bc.encode(s) for s in every))
        assert want[2] == (3 * len(every), 0, 0, 0)
        for missing in (every[0], every[-1], every[len(every) // 2]):
            want = _exact(rec, bclen, _white(bc.encode(s) for s in every if s != missing))
            assert want[2] == (3 * len(every) - 3, 0, 0, 3)                     # (its 3 x bclen neighbours are all listed)


# ---- 3. candidate counts ------------------------------------------------------------------------------------------------------------------------
def test_every_number_of_candidates():
    base = "ACGTTGCAACGTTGCA"
    cases = [   # the record's barcode, the whitelist entries near it, the status
        (base, [_sub(base, 5, 1)], 1),                                               # exactly one candidate
        (base, [_sub(base, 5, 1), _sub(base, 5, 2)], 3),                             # two at one position
        (base, [_sub(base, 9, 1), _sub(base, 9, 2), _sub(base, 9, 3)], 3),           # three at one position: all substitutions listed
        (base, [_sub(base, 1, 1), _sub(base, 6, 2)], 3),                             # two at different positions, one half
        (base, [_sub(base, 2, 3), _sub(base, 13, 1)], 3),                            # ... in different halves
        (base, [_sub(base, 0, 1), _sub(base, 15, 1)], 3),                            # ... the first and the last base
        (base, [_sub(base, 7, 2), _sub(_sub(base, 7, 2), 8, 1), _sub(_sub(base, 3, 1), 4, 1), _sub(_sub(base, 0, 3), 15, 3)], 1),      # one at 1 beside several at 2
        (base, [base, _sub(base, 4, 1), _sub(base, 11, 2)], 0),                      # listed, with neighbours listed too
        (base, [_sub(_sub(base, 4, 1), 11, 2)], 2),                                  # nothing nearer than two bases
    ]
    for k, (seq, near, status) in enumerate(cases):
        filler = ["".join(np.random.default_rng(k).choice(list(bc.BASES), size=16)) for _ in range(40)]
        filler = [f for f in filler if cc.distance(f, seq) > 2]
        rec = _rec([bc.encode(seq)] * 3 + [bc.encode(f) for f in filler[:5]], seed=k)
        want = _exact(rec, 16, _white(bc.encode(s) for s in near + filler))
        assert want[0][:3].tolist() == [status] * 3, k
    # all of them against one whitelist is one more case (the statuses follow from the checker)
    rec = _rec([bc.encode(s) for _, near, _ in cases for s in near] + [bc.encode(base)], seed=77)
    _exact(rec, 16, _white(bc.encode(s) for _, near, _ in cases[:6] for s in near))


# ---- 4. the directory and its buckets -------------------------------------------------------------------------------------------------------------
def _probe_records(rng, white, bclen, n_each=60):
    """Barcodes around a whitelist: entries (the first and the last among them), single-base changes of entries, and random ones."""
    w = white.tolist()
    pick = [w[0], w[-1]] + [w[int(j)] for j in rng.integers(0, len(w), size=n_each)]
    near = [bc.encode(_sub(bc.decode(v, bclen), int(rng.integers(bclen)), int(rng.integers(1, 4)))) for v in pick]
    rand = rng.integers(0, 1 << min(2 * bclen, 63), size=n_each, dtype=np.uint64).tolist()
    return _rec(pick + near + rand + [0, (1 << (2 * bclen)) - 1], seed=len(w))


@pytest.mark.parametrize("n_white", [BUSC_BISECT_LEN - 1, BUSC_BISECT_LEN, BUSC_BISECT_LEN + 1, 4 * BUSC_BISECT_LEN + 3])
def test_one_bucket_below_at_and_above_the_bisection_length(n_white):
    """Every entry shares the directory's prefix -- the leading bases are all A --: one bucket holds the whole list, read whole up to
    BUSC_BISECT_LEN entries and bisected beyond; every other bucket is empty, the last one too."""
    bits = dir_bits(n_white, 16)
    assert 0 < bits < 8
    rng = np.random.default_rng(n_white)
    white = _white(rng.choice(1 << 20, size=n_white, replace=False))                 # (bits 20 .. 31 are zero: prefix 0)
    assert len(white) == n_white and int(white[-1]) >> (32 - bits) == 0
    want = _exact(_probe_records(rng, white, 16), 16, white)
    assert want[2][0] >= 2 and want[2][1] > 0
    # ... and the same list in the last bucket: the first one is empty
    top = _white(int(v) | (0xFFF << 20) for v in white)
    want = _exact(_probe_records(rng, top, 16), 16, top)
    assert want[2][0] >= 2 and want[2][1] > 0


def test_entries_that_differ_in_the_leading_bits_alone_and_neighbours_in_the_first_and_the_last_bucket():
    bits = dir_bits(64, 16)
    assert bits == 4
    tail = bc.encode("GATTACAGATTACA")                                               # 14 bases under 2 leading ones = the 4 directory bits
    white = _white((p << 28) | tail for p in range(16))                              # every bucket holds exactly one entry
    rng = np.random.default_rng(4)
    want = _exact(_probe_records(rng, white, 16), 16, white)
    assert want[2][0] >= 2
    # buckets 0 ("AA") and 15 ("TT") alone hold an entry, every bucket between them is empty: "CA", "AC", "GA" are one base from the first,
    # "CT", "TC", "TG" from the last, "TA" and "AT" from both -- their neighbours fall into bucket 0 and into the last one --, "CC" and "GG" from neither
    ends = _white([tail, (15 << 28) | tail])
    heads = ["AA", "TT", "CA", "AC", "TA", "AT", "CT", "TC", "CC", "GG", "GA", "TG"]
    rec = _rec([(bc.encode(h) << 28) | tail for h in heads] + [(bc.encode(h) << 28) | (tail ^ 1) for h in heads], seed=2)
    want = _exact(rec, 16, ends)
    assert want[0][:len(heads)].tolist() == [0, 0, 1, 1, 3, 3, 1, 1, 2, 2, 1, 1]
    # two entries one base apart, in buckets 0 and 3 of 16
    near = _white([tail, (3 << 28) | tail])                                          # AA.. and AT..: buckets 0 and 3 of 16
    want = _exact(_rec([(1 << 28) | tail, (2 << 28) | tail, (7 << 28) | tail], seed=3), 16, near)
    assert want[0].tolist() == [3, 3, 1]


@pytest.mark.parametrize("b", list(range(0, 19)))
def test_whitelists_on_both_sides_of_every_directory_size(b):
    """n_white = BUSC_BUCKET_AVG << b is the last size with b directory bits, one more entry the first with b + 1; up to 2^20 random
    entries, a whitelist of a real kit's order of magnitude."""
    edge = BUSC_BUCKET_AVG << b
    assert dir_bits(edge, 16) == b and dir_bits(edge + 1, 16) == b + 1 and (b < 18 or edge == 1 << 20)
    rng = np.random.default_rng(b)
    pool = np.unique(rng.integers(0, 1 << 32, size=edge + 1 + edge // 8 + 64, dtype=np.uint64))
    assert len(pool) > edge
    pool = pool[rng.permutation(len(pool))[:edge + 1]]
    for n_white in (edge, edge + 1):
        white = np.sort(pool[:n_white])
        want = _exact(_probe_records(rng, white, 16, n_each=40), 16, white)
        assert want[2][0] >= 2 and (b < 3 or want[2][1] > 0)


# ---- 5. sizes -----------------------------------------------------------------------------------------------------------------------------------
def _size_world():
    """A whitelist of 40 barcodes at least 3 bases apart, and for each one barcode of every status but ambiguous; one ambiguous pair."""
    if "world" not in _kept:
        rng = np.random.default_rng(8)
        cells = []
        while len(cells) < 40:
            s = "".join(rng.choice(list(bc.BASES), size=16))
            if all(cc.distance(s, x) >= 4 for x in cells):
                cells.append(s)
        twin = _sub(cells[0], 3, 1)                                                  # listed too: cells[0] with base 3 changed again is ambiguous
        white = _white(bc.encode(s) for s in cells + [twin])
        wset = set(white.tolist())
        good = [bc.encode(s) for s in cells[1:]]
        fix = [bc.encode(_sub(s, k % 16, 1 + k % 3)) for k, s in enumerate(cells[1:])]
        lost = [bc.encode(_sub(_sub(s, 2, 1), 9, 2)) for s in cells[1:]]
        amb = bc.encode(_sub(cells[0], 3, 2))
        assert all(cc.outcome(v, 16, wset)[0] == 1 for v in fix) and all(cc.outcome(v, 16, wset)[0] == 2 for v in lost) and cc.outcome(amb, 16, wset)[0] == 3
        _kept["world"] = (white, np.array(good, dtype=np.uint64), np.array(fix, dtype=np.uint64), np.array(lost, dtype=np.uint64), amb)
    return _kept["world"]


def _by_status(status, seed):
    """Records with these statuses, in this order."""
    white, good, fix, lost, amb = _size_world()
    rng = np.random.default_rng(seed)
    status = np.asarray(status)
    j = rng.integers(0, len(good), size=len(status))
    bcs = np.where(status == 0, good[j], np.where(status == 1, fix[j], np.where(status == 2, lost[j], np.uint64(amb))))
    return _rec(bcs, seed=seed), white


@pytest.mark.parametrize("n", [1, TPB - 1, TPB, TPB + 1, SCB - 1, SCB, SCB + 1, 2 * SCB + 9])
def test_sizes(n):
    """n records of every status mixed -- with a run of misses across every workgroup's edge, the first and the last record dropped --, then
    all kept, none kept, and kept and dropped alternating."""
    rng = np.random.default_rng(n)
    status = rng.choice(4, size=n, p=[0.6, 0.2, 0.15, 0.05])
    for edge in range(TPB, n, TPB):
        status[max(edge - 3, 0):edge + 3] = [1, 2, 3, 1, 2, 1][:len(status[max(edge - 3, 0):edge + 3])]
    status[0] = status[-1] = 2
    rec, white = _by_status(status, n)
    want = _exact(rec, 16, white)
    assert want[0].tolist() == status.tolist()
    for pattern in (np.zeros(n, dtype=int), np.ones(n, dtype=int), np.full(n, 2), np.arange(n) % 2 * 2, 3 - np.arange(n) % 2 * 3):
        rec, white = _by_status(pattern, n + 1)
        want = _exact(rec, 16, white, tensors=bool(n % 2))
        assert want[0].tolist() == pattern.tolist() and len(want[1]) == int((pattern <= 1).sum())


@pytest.mark.parametrize("n_miss", [0, 1, BUSC_LANES - 1, BUSC_LANES, BUSC_LANES + 1, TPB // BUSC_LANES + 1, "all"])
def test_miss_counts(n_miss):
    n = 3 * TPB + 5
    k = n if n_miss == "all" else n_miss
    status = np.zeros(n, dtype=int)
    at = np.random.default_rng(k).choice(n, size=k, replace=False)
    status[at] = 1 + np.arange(k) % 3
    rec, white = _by_status(status, k)
    want = _exact(rec, 16, white)
    assert want[2][0] == n - k and sum(want[2][1:]) == k


# ---- 6. one rule for every route ------------------------------------------------------------------------------------------------------------------
def _route_input():
    rng = np.random.default_rng(21)
    status = rng.choice(4, size=SCB + 77, p=[0.7, 0.15, 0.1, 0.05])
    return _by_status(status, 21)


def _digest(out):
    rec, status, sizes = out
    h = hashlib.sha256()
    for x in (rec, status, np.array(sizes, dtype=np.uint64)):
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def _routes():
    rec, white = _route_input()
    return [_digest(_library(rec, 16, white, tensors=tensors)) for tensors in (False, True)]


def test_the_host_entry_the_device_entry_and_a_second_call_give_the_same_bytes():
    first, second = _routes(), _routes()
    assert first[0] == first[1] and first == second
    _kept["routes"] = first
    rec, white = _route_input()
    want = _exact(rec, 16, white)
    for tensors in (False, True):                                                    # want_status off: the same records
        out, status, sizes = _library(rec, 16, white, tensors=tensors, want_status=False)
        assert status is None and sizes == want[2] and np.array_equal(out, want[1])


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bytes():
    if "routes" not in _kept:
        _kept["routes"] = _routes()
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_buscorrect as t; print('digest', ' '.join(t._routes() + t._routes()))"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + " ".join(_kept["routes"] * 2) in r.stdout


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
PATTERN = 0x5C


class _Raw(object):
    """``ecb_bus_correct_device`` called by hand: inputs as CUDA tensors, outputs pre-filled with 0x5C at exactly the capacity."""

    def __init__(self, rec, white, bclen=16):
        import torch
        self.torch, self.lib = torch, ebc.load()
        self.rec, self.white, self.bclen, self.n = np.ascontiguousarray(rec).reshape(-1, 32), white, bclen, len(rec)

    def call(self, rec=None, white=None, cap=None, bclen=None, null=(), overlap=None, n_white=None):
        torch = self.torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy(), device="cuda")
        cap = self.n if cap is None else cap
        rec = self.rec if rec is None else rec
        white = self.white if white is None else white
        room = torch.full((self.n * 32 + max(cap, 1) * 32,), PATTERN, dtype=torch.uint8, device="cuda")
        room[:self.n * 32] = dev(rec)
        d_rec, d_out = room[:self.n * 32], room[self.n * 32:]
        if overlap is not None:                                                      # out begins `overlap` bytes before the records end
            d_out = room[self.n * 32 - overlap:self.n * 32 - overlap + max(cap, 1) * 32]
        d_white = dev(white)
        self.outs = [room[self.n * 32:], torch.full((self.n,), PATTERN, dtype=torch.uint8, device="cuda")]
        sizes = (C.c_uint64 * 4)(*[7] * 4)
        P = ecb._dev_ptr
        args = dict(rec=P(d_rec), white=P(d_white), out=P(d_out), status=P(self.outs[1]), sizes=sizes)
        for name in null:
            args[name] = None
        rc = self.lib.ecb_bus_correct_device(0, args["rec"], self.n, self.bclen if bclen is None else bclen, args["white"],
                                             len(white) if n_white is None else n_white, cap, args["out"], args["status"], args["sizes"])
        torch.cuda.synchronize()
        self.rec_after = room[:self.n * 32].cpu().numpy().reshape(-1, 32)
        return rc, tuple(sizes), (self.lib.ecb_last_error(None) or b"").decode()

    def untouched(self):
        return all(bool((o == PATTERN).all()) for o in self.outs)

    def result(self, n_out):
        return self.outs[0][:n_out * 32].cpu().numpy().reshape(-1, 32), self.outs[1].cpu().numpy()


def _raw_case():
    if "raw" not in _kept:
        status = np.random.default_rng(33).choice(4, size=2 * TPB + 9, p=[0.5, 0.25, 0.15, 0.1])
        rec, white = _by_status(status, 33)
        raw = _Raw(rec, white)
        rc, sizes, msg = raw.call()
        assert rc == 0, msg
        want = cc.correct(rec, 16, white)
        assert sizes == want[2]
        _kept["raw"] = (raw, want)
    return _kept["raw"]


def _good(raw, want, **kw):
    rc, sizes, msg = raw.call(**kw)
    assert rc == 0 and sizes == want[2], (rc, msg)
    out, status = raw.result(sizes[0] + sizes[1])
    assert np.array_equal(out, want[1]) and ("status" in kw.get("null", ()) or np.array_equal(status, want[0]))
    assert bool((raw.outs[0][len(want[1]) * 32:] == PATTERN).all())                  # nothing behind the records kept


def _refused(raw, want, code, text, **kw):
    rc, sizes, msg = raw.call(**kw)
    assert rc == code and text in msg, (rc, msg)
    assert sizes == (7,) * 4 and raw.untouched() and np.array_equal(raw.rec_after, kw.get("rec", raw.rec))
    _good(raw, want)


def _with_bc(rec, at, value):
    r = rec.copy().reshape(-1).view(cc._REC)
    for i in np.atleast_1d(at):
        r["bc"][i] = value
    return r.view(np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("at", ["first", "middle", "last", "two"])
def test_a_barcode_bit_too_high_is_refused_with_the_lowest_record(at):
    raw, want = _raw_case()
    where = {"first": [0], "middle": [raw.n // 2], "last": [raw.n - 1], "two": [raw.n - 3, TPB + 1]}[at]
    for value in (1 << 32, 1 << 63, (1 << 64) - 1):
        _refused(raw, want, CONTRACT, "bus: record %d: a barcode bit at or above 2 x bclen" % min(where), rec=_with_bc(raw.rec, where, value))


def test_a_malformed_whitelist_is_refused_with_the_lowest_entry():
    raw, want = _raw_case()
    w = raw.white
    falling = w.copy(); falling[[7, 8]] = falling[[8, 7]]
    equal = w.copy(); equal[20] = equal[19]
    both = falling.copy(); both[30] = both[29]
    high = w.copy(); high[-1] = np.uint64(1 << 32)
    high0 = w.copy(); high0[0] = np.uint64(1 << 63)                                  # (entry 0 has a bit too high; entry 1 is then not above it)
    for white, entry, why in ((falling, 8, "not above the entry before it"), (equal, 20, "not above the entry before it"),
                              (both, 8, "not above the entry before it"), (high, len(w) - 1, "a bit at or above 2 x bclen"),
                              (high0, 0, "a bit at or above 2 x bclen")):
        _refused(raw, want, CONTRACT, "bus: whitelist entry %d: %s" % (entry, why), white=white)
    with pytest.raises(ebc.WhitelistFormatError) as e:
        ebc.correct(raw.rec, 16, equal)
    assert (e.value.what, e.value.index, e.value.code) == ("whitelist entry", 20, CONTRACT)
    with pytest.raises(ecb_bus.BusFormatError) as e:
        ebc.correct(_with_bc(raw.rec, [40, 9], 1 << 40), 16, w)
    assert (e.value.what, e.value.index) == ("record", 9) and not isinstance(e.value, ebc.WhitelistFormatError)


def test_a_capacity_one_too_small_is_refused_and_the_exact_one_is_enough():
    raw, want = _raw_case()
    n_out = len(want[1])
    _good(raw, want, cap=n_out)
    _refused(raw, want, ARG, "%d records kept; room for %d" % (n_out, n_out - 1), cap=n_out - 1)
    _refused(raw, want, ARG, "room for 0", cap=0)
    with pytest.raises(ecb.EcbError) as e:
        ebc.correct(raw.rec, 16, raw.white, capacity=n_out - 1)
    assert e.value.code == ARG
    assert len(ebc.correct(raw.rec, 16, raw.white, capacity=n_out)[0]) == n_out


def test_bad_arguments_are_refused_before_anything_runs():
    raw, want = _raw_case()
    for kw, code in ((dict(bclen=0), ARG), (dict(bclen=33), ARG), (dict(null=("rec",)), ARG), (dict(null=("white",)), ARG), (dict(null=("out",)), ARG),
                     (dict(null=("sizes",)), ARG), (dict(n_white=0), ARG), (dict(overlap=1), ARG), (dict(overlap=32), ARG), (dict(overlap=raw.n * 32), ARG),
                     (dict(n_white=1 << 31), LIMIT)):
        rc, sizes, msg = raw.call(**kw)
        assert rc == code and msg.startswith("bus: ") and sizes == (7,) * 4 and raw.untouched() and np.array_equal(raw.rec_after, raw.rec), (kw, rc, msg)
    _good(raw, want, null=("status",))                                               # the status may be left out
    _good(raw, want, overlap=0)                                                      # out begins where the records end


def test_the_command_names_the_file_and_the_record(tmp_path):
    raw, want = _raw_case()
    lines = [[0], [0, 1]]
    rec = _with_bc(raw.rec, [300, 17], 1 << 32)
    rec.reshape(-1).view(cc._REC)["ec"] = 0
    rec.reshape(-1).view(cc._REC)["umi"] &= np.uint64(0xFFFF)
    d = bc.write_bus_dir(str(tmp_path / "bus"), rec, 16, 8, lines, ["t0_A", "t1_A"])
    wl = str(tmp_path / "wl.txt")
    with open(wl, "w") as fh:
        fh.write("".join(bc.decode(v, 16) + "\n" for v in raw.white))
    for run in (lambda: bus_utils.convert(d, str(tmp_path / "out.bin"), mincount=0, whitelist_file=wl),
                lambda: bus_utils.correct_file(os.path.join(d, "output.bus"), str(tmp_path / "out.bus"), wl)):
        with pytest.raises(ValueError) as e:
            run()
        assert "output.bus record 17: a barcode bit at or above 2 x bclen" in str(e.value) and str(e.value).count("record") == 1
    with open(wl, "a") as fh:
        fh.write("ACGTNCGTACGTACGT\n")
    with pytest.raises(ValueError) as e:
        bus_utils.convert(d, str(tmp_path / "out.bin"), mincount=0, whitelist_file=wl)
    assert "wl.txt line %d: barcode 'ACGTNCGTACGTACGT' has a letter outside ACGT" % (len(raw.white) + 1) in str(e.value)
    assert not os.path.exists(str(tmp_path / "out.bin")) and not os.path.exists(str(tmp_path / "out.bus"))


# ---- 8. downstream --------------------------------------------------------------------------------------------------------------------------------
def test_ecquant_cells_on_the_corrected_conversion_equals_ecquant_cells_on_the_golden_file(tmp_path):
    golden = os.path.join(GOLDEN, "g4_multi_min20.bin")
    m = bin_utils.ecload(os.path.join(GOLDEN, "g4_multi_min0.bin"))
    b, wl, damaged, white, head, n_one, n_two = _corrupted(m, str(tmp_path / "bus"), dict(split=True, shuffle=True), 6)
    out = str(tmp_path / "converted.bin")
    bus_utils.convert(b["dir"], out, mincount=20, names_file=b["names"], lengths_file=b["lengths"], whitelist_file=wl)
    tables = []
    for k, f in enumerate((out, golden)):
        table = str(tmp_path / ("cells%d.tsv" % k))
        bin_utils.ecquant_cells(f, table, use_lengths=True, max_iters=50)
        with open(table, "rb") as fh:
            tables.append(fh.read())
    assert tables[0] == tables[1] and len(tables[0]) > 1000
