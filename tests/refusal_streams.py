"""The streams of ``test_gpu_refused_runs.py``: for every place of libecb that answers ECB_ERR_TABLE_FULL because the key arena ran out, a
stream that must exhaust an arena of ``ARENA`` pairs however the waves pack their chunks, and a recovery stream that must fit it.  Made on
the CPU from ``alntools_amd/synth.py``'s counter-based random numbers (a pure function of the seed), in the tuple form of ``include/ecb.h``.

The margins are conditions on the streams, computed from constants read out of the kernel sources (as ``test_threshold_constants.py``
reads them), not measurements of the library:

* refused: the distinct keys alone -- ``sum(max(0, pairs - INL))`` over the distinct target sets, the part of a key that does not fit its
  table slot -- need at least ``4 * ARENA`` pairs;
* recovery: the same sum, plus one ``ARENA_CHUNK`` for every wave a batch of the whole stream can launch (``plan_stream``: at most
  ``ceil(n / (2 * WT))``), is at most ``ARENA / 4``.

``test_refusal_streams.py`` (CPU) asserts both on every stream, with the tuple contract and the C oracle's acceptance."""
import os
import re

import numpy as np

from alntools_amd import synth
from oracle import ec_oracle as orc

from tuple_contract import obeys_contract              # (the streams of contract_streams.py are held to it too)

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")
ARENA = 4096                     # arena_capacity of the handle that is refused: one region, eight ARENA_CHUNKs
SEED = 77
ARENA_REGIONS_RULE = (r"arena_regions\(u64 arena_cap\) \{ return \(u32\)\(arena_cap >> 16 >= ARENA_REGIONS \? ARENA_REGIONS : "
                      r"\(arena_cap >> 16 \? arena_cap >> 16 : 1\)\); \}")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _definition(fname, name):
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, _source(fname))
    assert len(defs) == 1, "%s: %d definitions of %s" % (fname, len(defs), name)
    return defs[0].strip()


def _constants():
    c = {k: int(_definition("ecb.hip", k)) for k in ("INL", "ARENA_CHUNK", "ARENA_REGIONS")}
    wt = re.fullmatch(r"64 \* RPL", _definition("ecb.hip", "WT"))
    rpl = re.search(r"#ifndef ECB_RPL\s*\n#define ECB_RPL (\d+)\b", _source("ecb.hip"))
    assert wt and rpl and _definition("ecb.hip", "RPL") == "ECB_RPL", "WT is no longer 64 * ECB_RPL: restate it here"
    c["WT"] = 64 * int(rpl.group(1))
    cmax = re.fullmatch(r"KS_SHORT \? (\d+) : (\d+)", _definition("k_stream.inc", "CMAX"))
    assert cmax, "CMAX is no longer `KS_SHORT ? a : b`: restate it here"
    c["CMAX_SHORT"], c["CMAX"] = int(cmax.group(1)), int(cmax.group(2))
    return c


_C = _constants()
INL, ARENA_CHUNK, ARENA_REGIONS, WT, CMAX, CMAX_SHORT = (_C[k] for k in ("INL", "ARENA_CHUNK", "ARENA_REGIONS", "WT", "CMAX", "CMAX_SHORT"))


def arena_regions(arena_cap):
    """``ecb.hip: arena_regions`` (the line is pinned by ``test_refusal_streams.py``): regions of at least 2^16 pairs, at most ARENA_REGIONS."""
    return min(ARENA_REGIONS, max(arena_cap >> 16, 1))


# ---- what a stream asks of the arena ----------------------------------------------------------------------------------------------------
def read_keys(t):
    """-> one key per read, in read order: the sorted tuple of (locus, haplotype mask) over the read's valid records."""
    v = orc.tuples_valid(t["hapflag"])
    rid, loc = t["read_id"][v].astype(np.int64), t["locus"][v].astype(np.int64)
    hap = (t["hapflag"][v].astype(np.int64) >> 16) & 0xFF
    cuts = np.flatnonzero(np.diff(rid)) + 1
    keys = []
    for a, z in zip(np.r_[0, cuts], np.r_[cuts, len(rid)]):
        d = {}
        for l, h in zip(loc[a:z].tolist(), hap[a:z].tolist()):
            d[l] = d.get(l, 0) | (1 << h)
        keys.append(tuple(sorted(d.items())))
    return keys


def key_pairs_beyond_the_slot(t):
    """Pairs the distinct keys of ``t`` need in the arena: sum(max(0, pairs - INL))."""
    return sum(max(0, len(k) - INL) for k in set(read_keys(t)))


def recovery_need(t):
    """Pairs a push of ``t`` in one batch can take from the arena at most, up to the waste of chunks that end early (which the margin of
    four covers): one ARENA_CHUNK per wave of the launch, and the pairs themselves."""
    n = len(t["read_id"])
    return (n + 2 * WT - 1) // (2 * WT) * ARENA_CHUNK + key_pairs_beyond_the_slot(t)


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def _rnd(a, k, mod):
    return (synth._pos(synth._rnd(SEED, np.asarray(a, np.int64), k)) % mod).astype(np.int64)


def _stream(bases, lengths, n_haps, salt, stride=1):
    """Read r: ``lengths[r]`` records on the distinct loci bases[r], bases[r] + stride, ..., record i on a haplotype drawn from (salt, bases[r], i)."""
    lengths = np.asarray(lengths, np.int64)
    rid = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    i = np.arange(len(rid), dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    base = np.repeat(np.asarray(bases, np.int64), lengths)
    loc = base + i * stride
    hap = _rnd(base * 4096 + i, salt, n_haps)                  # (of the base, not of the read: two reads on one base share their key)
    rev = _rnd(rid * 4096 + i, salt + 1, 2)
    return dict(read_id=rid.astype(np.uint32), locus=loc.astype(np.uint32), hapflag=((hap << 16) | (rev << 4)).astype(np.uint32),
                pos=_rnd(rid * 4096 + i, salt + 2, 100000).astype(np.int32), n_reads=len(lengths))


class Case(object):
    """One arena site: handle shape, the stream that is refused and the stream that recovers."""

    def __init__(self, name, n_loci, n_haps, refused, recovery):
        self.name, self.n_loci, self.n_haps, self._refused, self._recovery, self._made = name, n_loci, n_haps, refused, recovery, {}

    def _get(self, which, make):
        if which not in self._made:
            self._made[which] = make(self)
        return self._made[which]

    @property
    def refused(self):
        return self._get("refused", self._refused)

    @property
    def recovery(self):
        return self._get("recovery", self._recovery)


# The stream kernel founding long keys (ks_std, with and without ranges): 600 distinct reads on 40 consecutive loci each -- 35 pairs of
# every key go to the arena, 21 000 in all -- and every third read once more, so that counts differ.  Recovery: 12 such reads, 8 of them
# twice, and a few short ones: one wave, 420 pairs.
LONG = 8 * INL


def _long_keys(n_keys, n_loci, n_haps, salt, short=0):
    order = np.r_[np.arange(n_keys), np.arange(0, n_keys, 3) if n_keys > 12 else np.arange(8)]
    order = order[np.argsort(_rnd(np.arange(len(order)), salt + 5, 1 << 30), kind="stable")]       # (repeats anywhere among the firsts)
    bases = np.r_[order * (LONG + 1), _rnd(np.arange(short), salt + 6, n_loci - INL)]
    lengths = np.r_[np.full(len(order), LONG), 1 + _rnd(np.arange(short), salt + 7, INL)]
    return _stream(bases, lengths, n_haps, salt)


STD = Case("std", 30_000, 4, lambda c: _long_keys(600, c.n_loci, c.n_haps, 100), lambda c: _long_keys(12, c.n_loci, c.n_haps, 200, short=20))

# Keys of INL + 1 pairs (ks_short with the reads hinted, ks_par forced): 16 500 distinct reads of six consecutive loci, one pair each in the
# arena -- more than four arenas by themselves, and every wave reserves a whole ARENA_CHUNK for its first one.  Recovery: 150 of them.
SHORT_LOCI = 16_500 * (INL + 2)
SHORT = Case("short", SHORT_LOCI, 8,
             lambda c: _stream(np.arange(16_500) * (INL + 2), np.full(16_500, INL + 1), c.n_haps, 300),
             lambda c: _stream(_rnd(np.arange(150), 401, 16_500) * (INL + 2), np.full(150, INL + 1), c.n_haps, 400))

# k_slow: 32 distinct reads of 600 loci -- longer than a tile, so the stream kernel defers every one of them -- 595 pairs each in the arena.
# Recovery: one read of WT + 1 loci (still longer than a tile: WT + 1 - INL pairs and one wave's chunk are within the quarter) among short ones.
SLOW_LEN = WT + 88
SLOW = Case("slow", 40_000, 4,
            lambda c: _stream(np.arange(32) * (SLOW_LEN + 1), np.full(32, SLOW_LEN), c.n_haps, 500),
            lambda c: _stream(np.r_[7, 100, 3000, 20_000, 9], np.r_[3, INL, WT + 1, 2, 1], c.n_haps, 600))

CASES = {c.name: c for c in (STD, SHORT, SLOW)}


def queue_stream():
    """The tight side of ``plan_stream``'s ``need_q`` ("a read with more than CMAX loci takes more than CMAX records"): 300 reads of
    CMAX + 1 distinct loci each, the shortest a read can be and still be deferred -- which it is when it holds a tile's last record with
    all its entries made (the kernel sees the next read's head only in the next tile).  Every tile is padded with unmapped records in front
    so that its last read ends on the tile's end.  -> (tuples, n_loci, n_haps)."""
    n, T, H = 300, 50_000, 4
    per = WT // (CMAX + 1)                                        # reads of a tile
    t = _stream(_rnd(np.arange(n), 701, T - CMAX - 1), np.full(n, CMAX + 1), H, 700)
    pad = WT - per * (CMAX + 1)
    out = {k: [] for k in ("read_id", "locus", "hapflag", "pos")}
    for r0 in range(0, n, per):
        a, z = r0 * (CMAX + 1), min(r0 + per, n) * (CMAX + 1)
        out["read_id"] += [np.full(pad, (r0 - 1) & 0xFFFFFFFF, np.uint32), t["read_id"][a:z]]      # (an unmapped record carries the latest read's number)
        out["locus"] += [np.zeros(pad, np.uint32), t["locus"][a:z]]
        out["hapflag"] += [np.full(pad, 4, np.uint32), t["hapflag"][a:z]]
        out["pos"] += [np.full(pad, -1, np.int32), t["pos"][a:z]]
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["n_reads"] = n
    return out, T, H
