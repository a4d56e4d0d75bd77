"""Streams laid out on the slices of one ``k_stream`` launch, so that every wave of the launch is at the same claim of the EC table at the
same moment (``test_gpu_racing_founders.py``; judged without a GPU by ``test_racing_streams.py``).

``plan_stream`` (``alntools_amd/csrc/ecb.hip``) cuts a batch of n records into
``min(resident waves x rounds, max(n / (min_tiles x WT), resident waves), ceil(n / (2 x WT)))`` slices of ``ceil(n / slices)`` records,
rounded up to whole tiles.  With n a multiple of 2 x WT = 1024 and n / 1024 <= 256 that is n / 1024 slices of exactly 1024 records, whatever
``ECB_ROUNDS`` (at least 1) and ``ECB_MIN_TILES`` (at least 2) are: the fewest resident waves the plan can assume is 256 CUs x 1 workgroup x 4
waves = 1024, so the middle term is the resident waves and the last one, n / 1024 <= 256, is the smallest.  All slices are resident at once
(four to a workgroup), and a slice whose first record is a read's first starts its wave on that read.

A race cannot be forced; a stream whose every slice founds the same ECs in the same order makes it the common case.  The families:

  same_order   every slice holds the same new keys of 1 - 3 records in the same order
  rotated      slice s holds slice 0's reads rotated by s passes of 64 reads: what one wave founds, the others look up a little earlier or later
  same_slot    pairs of keys (A, C) of different hashes on one slot of a 1024-slot table; even slices bring A first, odd slices C
  same_hash    the committed 64-bit collisions (F2, N23) padded to 2, 6 and 17 pairs: even slices found key A, odd slices key B, at the same place
  long_keys    keys of 6, 16, 17 and 40 pairs (the pairs past INL = 5 live in the key arena) among short ones, the same in every slice
  giants       the first read of every slice covers the slice's first tile with the same CMAX_STD + 1 = 81 loci ("loci81"), or with a colliding
               pair padded to 81 pairs, A in even slices and B in odd ones ("colliding"): open at the tile's end with more entries than a pass
               carries and the tile full, so the pass is flushed there (81 + 512 > WT + CMAX) and the read goes to k_slow, in every slice
  growth       3 000 distinct keys in six blocks, slice s holds block s mod 6: more ECs than a table of 1024 slots holds
  ranges       same_order with a reference_start per record that depends on the slice

A key is ``(loci, masks)``, two tuples; a read is ``(loci, haps)``, two int64 arrays, one record per set haplotype bit."""
import numpy as np

import set_hash as sh

WT = 512                        # records per tile (ecb.hip: WT)
SLICE = 2 * WT                  # records per slice of a launch the restatement covers
MAX_SLICES = 256                # 256 CUs x 1 workgroup x 4 waves = 1024 resident waves at the least: 256 slices are far inside
PASS = 64                       # reads per pass of ks_std and ks_par (k_stream.inc: WMAXR; ks_short takes 128)
CMAX_STD = 80                   # entries a read may carry over a flush (k_stream.inc: CMAX)
CAP_SMALL = 1024                # the smallest EC table

FX = sh.load()
T = FX["n_loci"]
H = 8
assert FX["families"]["F2"]["n_haps"] == H == FX["families"]["N23"]["n_haps"]


def plan_slices(n, res_waves=1024, rounds=24, min_tiles=32):
    """``plan_stream``'s (slices, chunk) for a batch of n records, line by line (ecb.hip: ``u64 waves = ...`` to ``waves = (n + chunk - 1) / chunk``)."""
    waves = min(res_waves * rounds, max(n // (min_tiles * WT), res_waves))
    waves = min(waves, (n + 2 * WT - 1) // (2 * WT))
    waves = max(waves, 1)
    chunk = (n + waves - 1) // waves
    chunk = (chunk + WT - 1) // WT * WT
    waves = (n + chunk - 1) // chunk
    return waves, chunk


def aligned_slices(n):
    """The number of slices of a batch the builder made: n / 1024 of 1024 records each, for every plan the library can come to."""
    assert n % SLICE == 0 and 1 <= n // SLICE <= MAX_SLICES, n
    return n // SLICE


# ---- keys and reads ------------------------------------------------------------------------------------------------------------------------
def hash_of(key):
    return sh.set_hash(np.array(key[0]), np.array(key[1]))


def key_of(loci, masks):
    o = np.argsort(np.asarray(loci), kind="stable")
    return tuple(int(np.asarray(loci)[i]) for i in o), tuple(int(np.asarray(masks)[i]) for i in o)


def read_of(key, order="asc"):
    return sh.read_of((np.array(key[0], np.int64), np.array(key[1], np.int64)), order)


def short_keys(rng, n, lengths=(1, 2, 3), weights=None, taken=()):
    """n distinct keys of 1 - 3 records: that many loci anywhere among the T, one haplotype bit each."""
    out, seen = [], set(taken)
    while len(out) < n:
        k = int(rng.choice(lengths, p=weights))
        loci = sorted(set(rng.integers(0, T, k).tolist()))
        key = (tuple(loci), tuple(1 << int(h) for h in rng.integers(0, H, len(loci))))
        if key not in seen:
            seen.add(key)
            out.append(key)
    return out


def long_key(rng, n):
    """A key of n pairs on n loci anywhere, one haplotype bit each."""
    loci = sorted(rng.choice(T, n, replace=False).tolist())
    return tuple(loci), tuple(1 << int(h) for h in rng.integers(0, H, n))


def covering(read, n=WT):
    """The records of `read` repeated round to n records: the same target set (duplicate records vanish), a whole tile long."""
    return np.resize(read[0], n), np.resize(read[1], n)


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
def build(slices, pos=None):
    """slices: one list of reads per slice.  Every slice is padded to exactly 1024 records with whole reads, each a repeat of a read the slice
    already holds (taken round from its first read on, the ones that still fit), so padding founds nothing.
    -> dict(read_id, locus, hapflag, n_reads, n_slices, slice_reads [reads per slice, padding included][, pos]); pos: f(slice, record index
    within the slice, locus) -> reference_start."""
    rid, loc, hf, ps, per = [], [], [], [], []
    r = 0
    for s, reads in enumerate(slices):
        reads = list(reads)
        n = sum(len(x[0]) for x in reads)
        assert 0 < n <= SLICE, "slice %d holds %d records" % (s, n)
        base, i, idle = list(reads), 0, 0
        while n < SLICE:
            x = base[i % len(base)]
            i += 1
            if len(x[0]) <= SLICE - n:
                reads.append(x)
                n += len(x[0])
                idle = 0
            else:
                idle += 1
                assert idle <= len(base), "slice %d: no read of at most %d records to pad with" % (s, SLICE - n)
        at = 0
        for x in reads:
            k = len(x[0])
            rid.append(np.full(k, r, np.uint32))
            loc.append(np.asarray(x[0], np.uint32))
            hf.append(np.asarray(x[1], np.uint32) << 16)
            if pos is not None:
                ps.append(np.array([pos(s, at + q, int(x[0][q])) for q in range(k)], np.int32))
            r += 1
            at += k
        per.append(len(reads))
    t = dict(read_id=np.concatenate(rid), locus=np.concatenate(loc), hapflag=np.concatenate(hf).astype(np.uint32), n_reads=r,
             n_slices=len(slices), slice_reads=per)
    if pos is not None:
        t["pos"] = np.concatenate(ps)
    assert_aligned(t)
    return t


def assert_aligned(t):
    """Every slice of the launch starts on a read's first record and ends on a read's last."""
    rid = t["read_id"]
    S = aligned_slices(len(rid))
    assert S == t["n_slices"] and plan_slices(len(rid)) == (S, SLICE)
    starts = np.arange(1, S) * SLICE
    assert (rid[starts] != rid[starts - 1]).all()
    assert (np.diff(rid.astype(np.int64)) >= 0).all() and rid[0] == 0 and int(rid[-1]) + 1 == t["n_reads"]


def slice_keys(t, s):
    """The keys of slice s's reads, in order."""
    a, z = s * SLICE, (s + 1) * SLICE
    rid, loc, hap = t["read_id"][a:z], t["locus"][a:z], t["hapflag"][a:z] >> 16
    out = []
    for r in range(int(rid[0]), int(rid[-1]) + 1):
        m = {}
        for l, h in zip(loc[rid == r].tolist(), hap[rid == r].tolist()):
            m[l] = m.get(l, 0) | 1 << h
        out.append((tuple(sorted(m)), tuple(m[l] for l in sorted(m))))
    return out


# ---- the families --------------------------------------------------------------------------------------------------------------------------
def same_order(S=64, seed=101, pos=None):
    rng = np.random.default_rng(seed)
    keys = short_keys(rng, 300)
    reads = [read_of(k) for k in keys]
    return build([reads] * S, pos=pos), dict(keys=keys, n_ecs=300)


def rotated(S=64, seed=103):
    rng = np.random.default_rng(seed)
    keys = short_keys(rng, 300)
    reads = [read_of(k) for k in keys]
    sl = []
    for s in range(S):
        k = (s * PASS) % len(reads)
        sl.append(reads[k:] + reads[:k])
    return build(sl), dict(keys=keys, n_ecs=300)


def slot_pairs(rng, n, cap=CAP_SMALL):
    """n pairs of short keys (A, C): different hashes, the same slot of a table of `cap` slots, every pair on a slot of its own."""
    by_slot = {}
    for k in short_keys(rng, 6000):
        by_slot.setdefault(hash_of(k) & (cap - 1), []).append(k)
    pairs = [tuple(v[:2]) for v in by_slot.values() if len(v) >= 2]
    assert len(pairs) >= n
    return pairs[:n]


def same_slot(S=64, seed=107):
    rng = np.random.default_rng(seed)
    pairs = slot_pairs(rng, 150)
    even = [read_of(k) for a, c in pairs for k in (a, c)]
    odd = [read_of(k) for a, c in pairs for k in (c, a)]
    return build([odd if s & 1 else even for s in range(S)]), dict(pairs=pairs, n_ecs=300)


COLLISION_LENGTHS = (2, 6, 17)       # inline | one pair in the arena | beyond RANKED_MAX = 16


def colliding_pairs(n_inst=4, fams=("F2", "N23")):
    """`n_inst` instances of each family, padded to 2, 6 and 17 pairs (N23's key b holds one more) -> [(key a, key b)]."""
    out = []
    for fam in fams:
        for i in range(n_inst):
            for li, n in enumerate(COLLISION_LENGTHS):
                ka, kb = sh.pad(FX["families"][fam]["collisions"][i], n, ("low", "mid", "high")[(i + li) % 3], FX)
                out.append((key_of(*ka), key_of(*kb)))
    return out


def same_hash(S=64, seed=109):
    rng = np.random.default_rng(seed)
    pairs = colliding_pairs()
    fill = [read_of(k) for k in short_keys(rng, 100)]
    sl = []
    for s in range(S):
        reads, f = [], iter(fill)
        for a, b in pairs:                                    # (a short read between two colliding ones: the colliding reads spread over the passes)
            reads += [read_of(b if s & 1 else a), next(f), next(f)]
        sl.append(reads + list(f))
    return build(sl), dict(colliding=pairs, n_ecs=2 * len(pairs) + 100)


LONG_LENGTHS = (6, 16, 17, 40)       # one pair in the arena | RANKED_MAX | one past it | most of a carry list


def long_keys_of(rng):
    return [long_key(rng, n) for n in LONG_LENGTHS for _ in range(4 if n == 40 else 8)]


def long_keys(S=64, seed=113):
    rng = np.random.default_rng(seed)
    longs = long_keys_of(rng)
    shorts = short_keys(rng, 140)
    reads = []
    for i, k in enumerate(shorts):
        reads.append(read_of(k))
        if i % 5 == 2:
            reads.append(read_of(longs[i // 5]))
    assert len(longs) == 28 and sum(1 for r in reads if len(r[0]) > 5) == 28
    return build([reads] * S), dict(longs=longs, n_ecs=168)


def giants(kind, S=64, seed=127):
    """-> (tuples, info): info["n_long"] = the reads every compilation (and the exactness pass) sends to k_slow: one per slice."""
    rng = np.random.default_rng(seed)
    tail = [read_of(k) for k in short_keys(rng, 150)]           # the slice's second tile, the same in every slice: ordinary racing founders
    if kind == "loci81":
        g = long_key(rng, CMAX_STD + 1)
        heads = [covering(read_of(g))] * S
        info = dict(giants=[g], n_ecs=151)
    else:
        ka, kb = sh.pad(FX["families"]["F2"]["collisions"][5], CMAX_STD + 1, "mid", FX)
        ka, kb = key_of(*ka), key_of(*kb)
        heads = [covering(read_of(kb if s & 1 else ka)) for s in range(S)]
        info = dict(giants=[ka, kb], colliding=[(ka, kb)], n_ecs=152)
    info["n_long"] = S
    return build([[heads[s]] + tail for s in range(S)]), info


def growth(S=96, seed=131):
    rng = np.random.default_rng(seed)
    keys = short_keys(rng, 3000, weights=(0.4, 0.3, 0.3))
    blocks = [[read_of(k) for k in keys[b * 500:(b + 1) * 500]] for b in range(6)]
    return build([blocks[s % 6] for s in range(S)]), dict(keys=keys, n_ecs=3000)


def ranges(S=64, seed=101):
    """same_order with reference_start = a function of the slice and the record: every (locus, haplotype) gets S different positions, its
    minimum and maximum from different slices."""
    return same_order(S, seed, pos=lambda s, i, locus: 1000 + (s * 7919 + i * 31 + locus) % 100003)


def range_minmax(t):
    """numpy's per-(locus, haplotype) minimum and maximum of pos (all records are valid); untouched pairs keep (INT_MAX, INT_MIN)."""
    cell = t["locus"].astype(np.int64) * H + (t["hapflag"] >> 16).astype(np.int64)
    mn = np.full(T * H, np.iinfo(np.int32).max, np.int32)
    mx = np.full(T * H, np.iinfo(np.int32).min, np.int32)
    np.minimum.at(mn, cell, t["pos"])
    np.maximum.at(mx, cell, t["pos"])
    return mn, mx


FAMILIES = {
    "same_order": same_order, "same_order_256": lambda: same_order(S=256), "rotated": rotated, "same_slot": same_slot, "same_hash": same_hash,
    "long_keys": long_keys, "giants_loci81": lambda: giants("loci81"), "giants_colliding": lambda: giants("colliding"), "growth": growth,
    "ranges": ranges,
}
SMALL_TABLE = ("same_slot", "growth")            # families whose handle has ec_capacity = 1024
_made, _expected = {}, {}


def family(name, oracle=True):
    """(tuples, info[, the C oracle's result on the whole stream]) of a family: made once, shared, never changed."""
    if name not in _made:
        t, info = FAMILIES[name]()
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _made[name] = (t, info)
    if not oracle:
        return _made[name]
    if name not in _expected:
        from oracle import c_oracle
        t = _made[name][0]
        _expected[name] = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=4)
    return _made[name] + (_expected[name],)


# ---- shards for k_merge --------------------------------------------------------------------------------------------------------------------
N_SHARDS = 8


def merge_shard(seed=137):
    """The reads every one of the eight shards pushes: ~3 000 short keys, the long keys of `long_keys`, the F2 collisions at every length (both
    keys of a pair).  -> (tuples of one shard, info)."""
    rng = np.random.default_rng(seed)
    keys = short_keys(rng, 3000)
    longs = long_keys_of(rng)
    pairs = colliding_pairs(8, ("F2",))
    extra = longs + [k for p in pairs for k in p]
    reads = [read_of(k) for k in keys]
    for i, k in enumerate(extra):
        reads.insert((i * 37) % 2900 + i, read_of(k, "desc" if i & 1 else "asc"))
    rid = np.concatenate([np.full(len(r[0]), i, np.uint32) for i, r in enumerate(reads)])
    t = dict(read_id=rid, locus=np.concatenate([r[0] for r in reads]).astype(np.uint32),
             hapflag=(np.concatenate([r[1] for r in reads]).astype(np.uint32) << 16), n_reads=len(reads))
    return t, dict(colliding=pairs, longs=longs, n_ecs=3000 + len(extra))


def concatenated(t, k=N_SHARDS):
    """k shards of the same reads, one behind the other, with their read bases."""
    n = t["n_reads"]
    return dict(read_id=np.concatenate([t["read_id"] + np.uint32(i * n) for i in range(k)]), locus=np.tile(t["locus"], k),
                hapflag=np.tile(t["hapflag"], k), n_reads=k * n)
