"""True collisions of the EC table's 64-bit set hash -- two DIFFERENT target sets with the SAME hash -- through every path that finds or
inserts an EC by its hash and must then tell the keys apart.  The collisions are data (``tests/golden/hash_collisions.json``, found by
``tests/golden/make_hash_collisions.py``, checked on the CPU by ``test_hash_collisions.py``); the expected results come from the oracles
(``oracle.c_oracle`` compares keys with memcmp, ``oracle.ec_oracle`` with dicts: neither shares anything with the device hash), never
from the library.

Families: F2 -- two pairs against two pairs on four different loci; N23 -- two pairs against three (the sizes differ: ``v.n != np``,
``sn != n``, ``ListCmp::quick``); M2 -- two pairs against two on the SAME loci with other masks ("the locus is mine, the mask is not";
masks of 24 bits, so never through ks_short, whose masks are bytes).  ``set_hash.pad`` adds the same pairs to both keys: inline keys
(up to INL = 5 pairs), arena keys, keys beyond RANKED_MAX = 16, BIG_LDS = 2048 and of k_slow's lengths, all from one search.

That the collision is real ON THE DEVICE is asserted, not assumed: ``test_the_numpy_hash_is_the_device_hash`` ties ``set_hash.py`` to
``export_ec_keys_device``, and every stream test asserts that the two colliding ECs' exported hashes are EQUAL while their CSR rows
differ (``_witness``) -- a retune of the hash turns these red, not into a test of nothing.

The stored order of a key's pairs is the founder's entry-queue order, which a test cannot dictate: which stored position the differing
pairs take is covered by SPREAD, not by construction -- their loci are the lowest, middle or highest of the key, the founding read
lists its loci ascending or descending, either key founds, and several instances of every family are used.  Displaced pairs (a stored
locus whose first LDS place holds another (read, locus)) ARE placed by construction, in ``test_displaced_pairs_of_colliding_keys``.
Nothing here can force CMP_INCOMPLETE or ST_STUCK: those are races between a publisher and a reader, which
``test_gpu_racing_founders.py`` makes the common case with streams laid out on the slices of one launch."""
import numpy as np
import pytest

from alntools_amd import ecb
from oracle import c_oracle
from oracle import ec_oracle as orc

import bundle_checker as bchk
import ec_merge_checker as chk
import set_hash as sh
import test_gpu_multisample as tm
import test_gpu_thresholds as th
from test_gpu_parity import _check, _run_host
from test_gpu_thresholds import COMPILATIONS, _every_push
from verify_checker import misplaced

pytestmark = pytest.mark.gpu

FX = sh.load()
T = FX["n_loci"]
WT, SLOW_LDS = th.WT, th.SLOW_LDS
LENGTHS = (2, 5, 6, 9, 10, 17)             # INL = 5: inline | 6: one pair in the arena | 9, 10: ks_par's last group of four holds one and two | 17: RANKED_MAX + 1
WHERES = ("low", "mid", "high")
ORDERS = ("asc", "desc")
GROUPS = {"h8": ("F2", "N23"), "h24": ("M2",)}     # families that share a haplotype count share a stream


def _H(family):
    return FX["families"][family]["n_haps"]


def _n_inst(family):
    return len(FX["families"][family]["collisions"])


def _pair(family, i, n, where):
    return sh.pad(FX["families"][family]["collisions"][i % _n_inst(family)], n, where, FX)


def _row(key):
    return tuple(zip(key[0].tolist(), key[1].tolist()))


def _rows_of(ip, ix, da):
    return {tuple(zip(ix[a:z].tolist(), da[a:z].tolist())): e for e, (a, z) in enumerate(zip(ip[:-1].tolist(), ip[1:].tolist()))}


def _expect(t, H):
    """Both oracles, which must agree: the C one (memcmp on sorted keys) and the Python one (dict of tuples)."""
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=4)
    py = orc.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], T, H)
    for k in ("indptr", "indices", "data", "count"):
        assert np.array_equal(exp[k], py[k]), k
    return exp


def _device_hashes(b):
    import torch
    n = b.sizes["n_ecs"]
    keys = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    b.export_ec_keys_device(keys)
    return keys[:n].cpu().numpy().view(np.uint64)


def _assert_collide(hashes, rows, pairs):
    """Every (key a, key b) of `pairs`: two different rows of the result whose device hashes are equal (and the numpy hash)."""
    for ka, kb in pairs:
        ea, eb = rows[_row(ka)], rows[_row(kb)]
        assert ea != eb and int(hashes[ea]) == int(hashes[eb]) == sh.set_hash(*ka), (ka, kb)


def _witness(t, H, exp, pairs):
    """One plain handle over the stream == the oracle, and the colliding ECs collide on the device."""
    with ecb.EcBuilder(T, H) as b:
        b.push_device(*th._dev(t))
        s = b.finalize()
        _check(b.export(), s, exp)
        _assert_collide(_device_hashes(b), _rows_of(exp["indptr"], exp["indices"], exp["data"]), pairs)


def _std_par_only(monkeypatch):
    """M2's masks have 24 bits: ks_short holds masks in bytes (at most 8 haplotypes) and cannot take them."""
    monkeypatch.setattr(th, "COMPILATIONS", {k: COMPILATIONS[k] for k in ("std", "par")})


def test_the_numpy_hash_is_the_device_hash():
    """``set_hash.py`` == the kernels' hash: a few thousand random ECs of 1 .. 40 pairs and every padded collision key, hashed by k_stream
    (a table behind the result) and by ``k_row_keys`` (an assembled result, hashed from its CSR rows), against numpy row by row."""
    import torch
    from alntools_amd import dist as ecdist
    rng = np.random.default_rng(1)
    H = 8
    reads = []
    for _ in range(1500):
        n = int(rng.integers(1, 41))
        loci = rng.choice(T, size=n, replace=False)
        reads.append(sh.read_of((loci, rng.integers(1, 1 << H, n)), "asc"))
    for f in ("F2", "N23"):
        for i in range(_n_inst(f)):
            for key in _pair(f, i, LENGTHS[i % len(LENGTHS)], WHERES[i % 3]):
                reads.append(sh.read_of(key))
    t = th._stream(reads)
    exp = _expect(t, H)
    want = sh.row_hashes(exp["indptr"], exp["indices"], exp["data"])
    dev = torch.device("cuda:0")
    with ecb.EcBuilder(T, H) as b:
        b.push_device(*th._dev(t))
        s = b.finalize()
        _check(b.export(), s, exp)
        assert np.array_equal(_device_hashes(b), want)
        assert len(np.unique(want)) < len(want)                         # (the collisions are in it)
    part = ecdist.GpuEngine(ecb.EcBuilder(T, H), dev)
    part.b.push_device(*th._dev(t))
    a, v, n = part.counters()
    ne, npairs, _ = part.table_sizes()
    ent, prs = part.table_export(0)
    mid = ecdist.GpuEngine(ecb.EcBuilder(T, H), dev)
    mid.table_merge(ent, ne, prs, npairs)
    piece = mid.finalize_range(a, v, n)
    with ecb.EcBuilder(T, H) as root:
        ecdist.GpuEngine(root, dev).assemble_ranges([piece], a, v, n)
        _check(root.export(), root.sizes, exp)
        assert np.array_equal(_device_hashes(root), want)
    part.b.close()
    mid.b.close()


# ---- k_stream ------------------------------------------------------------------------------------------------------------------------------
def _combos(family, shift):
    """(n, where, order, b_first, instance): every (instance, n, where) at most once per stream, so that each pair FOUNDS its two ECs."""
    out = []
    for n in LENGTHS:
        for where in (WHERES if n > 2 else WHERES[:1]):              # (no padding at 2 pairs: nothing to place)
            k = 0
            for order in ORDERS:
                for b_first in (False, True):
                    out.append((n, where, order, b_first, (k + shift) % _n_inst(family)))
                    k += 1
    return out


def _shape_stream(family, shape, seed):
    """-> (tuples, [(key a, key b)], {row: reads} expected for shape c).
    a  the two colliding reads ADJACENT (same slice, same pass, same flush: the second meets the first as a freshly claimed slot of its
       own hash, ST_PENDING, or as a published key), either one first
    b  the same, the second read 200 tiles later (``plan_stream`` cuts a stream this small into slices of a few tiles, each walked by a
       wave of its own, unless ECB_ROUNDS / ECB_MIN_TILES say otherwise: the test takes them out of the environment): another wave, a
       slot long published
    c  each of the two 50 .. 200 times, interleaved at random: counts in N and first-appearance ranks, not only existence"""
    rng = np.random.default_rng(seed)
    H = _H(family)
    reads, pairs, counts = th._fill(rng, 300, T, H), [], {}
    later = []
    combos = _combos(family, {"a": 0, "b": 4, "c": 2}[shape])
    if shape == "c":
        combos = [combos[(7 * k) % len(combos)] for k in range(len(LENGTHS) + 2)]
        assert len({(c[0], c[1], c[4]) for c in combos}) == len(combos)
    for n, where, order, b_first, i in combos:
        ka, kb = _pair(family, i, n, where)
        pairs.append((ka, kb))
        ra, rb = sh.read_of(ka, order), sh.read_of(kb, order)
        first, second = (rb, ra) if b_first else (ra, rb)
        if shape == "a":
            reads += [first, second] + th._fill(rng, int(rng.integers(1, 40)), T, H)
        elif shape == "b":
            reads += [first] + th._fill(rng, int(rng.integers(1, 40)), T, H)
            later += [second] + th._fill(rng, int(rng.integers(1, 40)), T, H)
        else:
            na, nb = (int(x) for x in rng.integers(50, 201, 2))
            counts[_row(ka)], counts[_row(kb)] = na, nb
            seq = rng.permutation([0] * (na - (not b_first)) + [1] * (nb - b_first)).tolist()
            for which in [int(b_first)] + seq:
                reads.append(rb if which else ra)
                if rng.random() < 0.2:
                    reads += th._fill(rng, int(rng.integers(1, 10)), T, H)
    if shape == "b":
        reads += th._fill(rng, 200 * WT, T, H) + later
    reads += th._fill(rng, 300, T, H)
    return th._stream(reads), pairs, counts


@pytest.mark.parametrize("shape", ["a", "b", "c"])
@pytest.mark.parametrize("family", ["F2", "N23", "M2"])
def test_colliding_reads_through_every_compilation_and_push(family, shape, monkeypatch):
    """``table_lookup``'s fall-through, ``table_settle`` -> ST_OTHER and the probe-on behind it, and CMP_DIFFERENT out of
    ``LdsSetCmp::quick_lean`` (ks_std, ks_short), ``LdsSetCmp::quick`` (ks_par) and ``LdsSetCmp::full``: key lengths 2, 5, 6, 9, 10 and 17,
    the differing pairs lowest / middle / highest by locus, records ascending / descending, either key founding, in the stream shapes of
    ``_shape_stream``; through ``_every_push`` (every compilation forced, arrays and tiles, host pushes in odd batches, the exactness pass
    reporting 0) against the oracles.  The exactness pass (``k_stream<true>``) thereby compares every read with the right one of two ECs
    with one hash.  M2 on ks_std and ks_par only (24-bit masks)."""
    t, pairs, counts = _shape_stream(family, shape, 10 * len(family) + ord(shape))
    H = _H(family)
    exp = _expect(t, H)
    rows = _rows_of(exp["indptr"], exp["indices"], exp["data"])
    for r, c in counts.items():
        assert exp["count"][rows[r]] == c
    assert len(t["read_id"]) < 130_000
    monkeypatch.delenv("ECB_ROUNDS", raising=False)
    monkeypatch.delenv("ECB_MIN_TILES", raising=False)
    _witness(t, H, exp, pairs)
    if family == "M2":
        _std_par_only(monkeypatch)
    _every_push(t, T, H, exp, monkeypatch, n_long=(0, 0))


# ---- displaced pairs, by construction -------------------------------------------------------------------------------------------------
def _dense(t, least):
    """Every tile of the stream holds at least `least` read heads."""
    heads = np.flatnonzero(np.concatenate(([True], t["read_id"][1:] != t["read_id"][:-1])))
    per = np.bincount(heads // WT, minlength=(len(t["read_id"]) + WT - 1) // WT)
    return int(per[:-1].min()) >= least


@pytest.mark.parametrize("n", [4, 5, 6, 10, 17])
def test_displaced_pairs_of_colliding_keys(n, monkeypatch):
    """Stream shape (d): the founder's differing loci are DISPLACED in the other read's pass table.  ``set_hash.displace`` gives both keys,
    for every differing locus D of the founder, a padding locus P with ``home_off(P) == home_off(D)`` in a home region of 8 slots.  The
    other key's read holds P and not D, so where its lookup looks for the stored D first, another (read, locus) sits: not empty, not D
    with another mask -- nothing the quick compare can decide on.  That is ``quick_lean`` -> CMP_UNSURE for an inline D and at the arena
    loop for a stored D beyond INL (ks_std, ks_short) -> ``table_settle`` -> ``LdsSetCmp::full`` walking on to CMP_DIFFERENT -> ST_OTHER
    -> the next slot; and in ks_par ``quick``'s ``moved`` set, D looked for at its second place and -- that place empty or taken --
    CMP_DIFFERENT there or out of the ``far`` walk (which of the two is not constructed), and ``has()`` for a stored D in the arena.
    The founder's OWN later reads meet the same displaced pair on the equal side (P and D share a place in their table): CMP_UNSURE ->
    ``full`` -> CMP_EQUAL, and ks_par's second place -> equal.

    The region has 8 slots whenever the pass is laid out for as many reads as it can take: at a slice's start, and behind a flush whose
    last tile brought at least 16 reads (ks_std, ks_par) or 32 (ks_short) -- every tile of this stream brings 40 and more, which is
    asserted; ``test_hash_collisions.py`` pins the lines of ``k_stream.inc`` this rests on.  n = 4, 5: inline keys, the pads of the
    founder only (A founds one instance, B another); n = 6, 10, 17: the pads of both keys, either founding, differing pairs stored
    inline or in the arena as the founder's entry queue has it.  F2 only: N23 is decided by the sizes and M2 at D's first place (the
    locus is mine, the mask is not) before displacement can matter.  Through ``_every_push`` against the oracles."""
    rng = np.random.default_rng(300 + n)
    H = 8
    cols = FX["families"]["F2"]["collisions"]
    reads, pairs, again = th._fill(rng, 400, T, H), [], []
    for k, b_first in enumerate((False, True, False, True)):
        founder = ("b" if b_first else "a") if n < 6 else "ab"
        ka, kb = sh.displace(cols[(n + k) % len(cols)], n, founder, WHERES[k % 3], FX)
        assert sh.set_hash(*ka) == sh.set_hash(*kb)
        for own, other in (((kb, ka) if b_first else (ka, kb)),) + (((ka, kb), (kb, ka)) if n >= 6 else ()):
            diff = set(own[0].tolist()) - set(other[0].tolist())
            assert len(diff) == 2 and all(any(sh.home_off(d) == sh.home_off(p) for p in other[0].tolist()) for d in diff)
        pairs.append((ka, kb))
        ra, rb = sh.read_of(ka, ORDERS[k % 2]), sh.read_of(kb, ORDERS[(k // 2) % 2])
        reads += list((rb, ra) if b_first else (ra, rb)) + th._fill(rng, 60, T, H)
        again += [ra, rb, rb, ra][k % 2:] + th._fill(rng, 60, T, H)
    reads += th._fill(rng, 300, T, H) + again + th._fill(rng, 400, T, H)
    t = th._stream(reads)
    assert _dense(t, 40)
    exp = _expect(t, H)
    _witness(t, H, exp, pairs)
    _every_push(t, T, H, exp, monkeypatch, n_long=(0, 0))


# ---- k_slow --------------------------------------------------------------------------------------------------------------------------------
def _slow_stream(group, seed):
    """Colliding keys of CMAX + 1 = 65 (ks_short) and 81 (ks_std, ks_par) pairs, each read three times ENDING on a tile's end (open there
    with more than CMAX entries: deferred when the pass is flushed behind that tile, ``test_gpu_thresholds.py``'s header -- likely, not
    certain) and once with its records repeated round to 2 x WT + 1 (it covers a whole tile and is still open at its end with all its
    entries: ALWAYS deferred by the compilation whose CMAX it exceeds); of 1 100 pairs (covers a tile, always deferred; table in LDS) and,
    once, of 2 100 pairs (2 x records > SLOW_LDS: table in global scratch).  Either key founds.
    -> (tuples, pairs, reads certainly deferred by ks_std, reads it may defer)."""
    rng = np.random.default_rng(seed)
    H = _H(GROUPS[group][0])
    reads, at, pairs, sure, may = [], 0, [], 0, 0

    def add(r, tile_end):
        nonlocal at
        if tile_end:
            f = th._fill(rng, (-(at + len(r[0]))) % WT, T, H)
            reads.extend(f)
            at += sum(len(x[0]) for x in f)
        reads.append(r)
        at += len(r[0])
        assert not tile_end or at % WT == 0

    reads += th._fill(rng, 200, T, H)
    at += 200
    for fam in GROUPS[group]:
        for n in (65, 81, 1100):
            for b_first in (False, True):
                ka, kb = _pair(fam, n + b_first, n, "mid")
                pairs.append((ka, kb))
                ra, rb = sh.read_of(ka, "desc" if b_first else "asc"), sh.read_of(kb, "asc")
                for which in ((1, 0, 0, 1, 1, 0) if b_first else (0, 1, 1, 0, 0, 1)):
                    add(rb if which else ra, n < 1100)
                if n < 1100:                                             # ... and each once over a whole tile
                    for r in ((rb, ra) if b_first else (ra, rb)):
                        add((np.resize(r[0], 2 * WT + 1), np.resize(r[1], 2 * WT + 1)), False)
                sure += 6 * (n == 1100) + 2 * (n == 81)
                may += (6 + 2 * (n == 81)) * (n >= 81)
    fam = GROUPS[group][0]
    ka, kb = _pair(fam, 1, 2100, "mid")
    pairs.append((ka, kb))
    for which in (0, 1, 1, 0):
        add(sh.read_of(kb if which else ka), False)
    assert 2 * len(sh.read_of(ka)[0]) > SLOW_LDS
    reads += th._fill(rng, 700, T, H)
    return th._stream(reads), pairs, sure + 4, may + 4


@pytest.mark.parametrize("group", ["h8", "h24"])
def test_colliding_reads_through_k_slow(group, monkeypatch):
    """``k_slow``'s ``same_key`` returning CMP_DIFFERENT and the ``s_j + 1`` step behind it, with the read's table in LDS and in global
    scratch, and the exactness pass in k_slow's verify mode: ``_slow_stream`` through every compilation and push against the oracles.
    ``verify_device``'s second figure (the reads the exactness pass, ks_std with CMAX = 80, sent to k_slow) shows that the reads did go
    there: all of those that cover a tile with 81 pairs and more, and at least one of those that end on a tile's end with 81 and 82 pairs
    (a flush there is likely, not certain: as weak as ``test_gpu_thresholds.py``'s own witness for that shape).  The 65- and 66-pair
    reads exceed only ks_short's CMAX = 64: those that cover a tile are deferred by ks_short for certain by the same reading of the code
    (``k_stream.inc``: ``giant``), but no figure the library returns shows it -- the exactness pass carries them."""
    t, pairs, sure, may = _slow_stream(group, 77)
    H = _H(GROUPS[group][0])
    exp = _expect(t, H)
    _witness(t, H, exp, pairs)
    if group == "h24":
        _std_par_only(monkeypatch)
    _every_push(t, T, H, exp, monkeypatch, batches=(4097,), n_long=(sure + 1, may))


# ---- growth --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("verify", [False, True])
def test_colliding_ecs_stay_two_through_table_growth(verify):
    """``k_rehash`` with two live slots of one hash, ``k_remap_read_slot`` keeping the earlier reads apart: ``ec_capacity=64`` (1 024
    slots), colliding pairs of every family's length class founded in the first batch, then twice 4 000 filler reads (some 3 500 new ECs
    each: the table has to grow more than twice) with reads of both keys after each; counts and ranks == the oracles; and the same on a
    handle that runs the exactness pass after every batch (``verify=True``)."""
    rng = np.random.default_rng(5)
    H = 8
    pairs = [_pair(f, 5 + k, n, WHERES[k % 3]) for k, (f, n) in enumerate((f, n) for f in ("F2", "N23") for n in (2, 5, 6, 17))]
    batches = []
    for rnd in range(3):
        reads = [] if rnd == 0 else [th._distinct(rng, int(rng.integers(2, 9)), T, H) for _ in range(4000)]
        for k, (ka, kb) in enumerate(pairs):
            order = [ka, kb, kb, ka] if (k + rnd) % 2 else [kb, ka, ka]
            reads += [sh.read_of(x, ORDERS[(k + rnd) % 2]) for x in order] + th._fill(rng, 5, T, H)
        batches.append(reads)
    t = th._stream([r for b in batches for r in b])
    exp = _expect(t, H)
    assert len(exp["count"]) > 6 * 1024
    cuts = np.cumsum([0] + [sum(len(r[0]) for r in b) for b in batches])
    with ecb.EcBuilder(T, H, ec_capacity=64, verify=verify) as b:
        for a, z in zip(cuts[:-1], cuts[1:]):
            b.push(t["read_id"][a:z], t["locus"][a:z], t["hapflag"][a:z])
        s = b.finalize()
        _check(b.export(), s, exp)
        _assert_collide(_device_hashes(b), _rows_of(exp["indptr"], exp["indices"], exp["data"]), pairs)
        rows = _rows_of(exp["indptr"], exp["indices"], exp["data"])
        read_ec = b.export_read_ec()
    # every read of a colliding key sits in its own EC, the ones pushed before a growth too
    lens = np.bincount(t["read_id"].astype(np.int64))
    starts = np.cumsum(lens) - lens
    for ka, kb in pairs:
        for key in (ka, kb):
            loci, haps = sh.read_of(key, "asc")
            mine = [r for r in range(len(lens)) if lens[r] == len(loci) and
                    sorted(zip(t["locus"][starts[r]:starts[r] + lens[r]].tolist(), (t["hapflag"][starts[r]:starts[r] + lens[r]] >> 16).tolist())) == sorted(zip(loci.tolist(), haps.tolist()))]
            assert len(mine) == exp["count"][rows[_row(key)]] >= 4 and (read_ec[mine] == rows[_row(key)]).all()


# ---- the exactness pass --------------------------------------------------------------------------------------------------------------------
def _swap(t, r, key):
    """`t` with the records of read r replaced by a read of `key` (no more records than r has: the rest repeat its first record)."""
    a, z = (int(x) for x in np.searchsorted(t["read_id"], [r, r + 1]))
    loci, haps = sh.read_of(key)
    assert len(loci) <= z - a
    loci = np.concatenate([loci, np.full(z - a - len(loci), loci[0])])
    haps = np.concatenate([haps, np.full(z - a - len(haps), haps[0])])
    out = dict(t)
    out["locus"], out["hapflag"] = t["locus"].copy(), t["hapflag"].copy()
    out["locus"][a:z], out["hapflag"][a:z] = loci, (haps << 16)
    return out


@pytest.mark.parametrize("family", ["F2", "N23", "M2"])
def test_the_exactness_pass_counts_a_read_that_sits_in_the_other_ec_of_its_hash(family):
    """A stream with reads of both keys is pushed; then ``verify_device`` is shown the same stream with ONE read of one key holding the
    records of the other: exactly 1 mismatch, which is also what ``verify_checker.misplaced`` counts, through the array form and the tiled
    form, for inline and arena keys (``k_stream<true>``) and for k_slow's lengths (81 pairs ending on a tile's end, 1 100 and 2 100
    pairs; its verify mode).  The exactness pass never looks a read up by its hash -- it takes the slot the push recorded for the read
    (``read_slot``) and compares keys -- so the equal hash plays no part in THIS compare: the case is a tampered read of (nearly) equal
    length, as in ``test_gpu_exactness_pass.py``.  What the collision adds is on the push side: the slot recorded for every untouched
    read of the two keys is the right one of two with one hash, or ``verify_device`` on the unchanged stream would not report 0."""
    rng = np.random.default_rng(9)
    H = _H(family)
    lengths = (2, 5, 6, 17, 81, 1100, 2100) if family != "M2" else (2, 5, 6, 17, 81)
    reads, at, targets = th._fill(rng, 300, T, H), 300, []
    for k, n in enumerate(lengths):
        ka, kb = _pair(family, 3 + k, n, WHERES[k % 3])
        ra, rb = sh.read_of(ka), sh.read_of(kb)
        big, small, small_key = (ra, rb, kb) if len(ra[0]) >= len(rb[0]) else (rb, ra, ka)
        for x in (ra, rb, big, small, big):
            if n == 81:
                f = th._fill(rng, (-(at + len(x[0]))) % WT, T, H)
            else:
                f = th._fill(rng, int(rng.integers(1, 30)), T, H)
            reads += f + [x]
            at += sum(len(q[0]) for q in f) + len(x[0])
        targets.append((len(reads) - 1, small_key, n))                  # the last read of the longer key will show the other key
    reads += th._fill(rng, 300, T, H)
    t = th._stream(reads)
    exp = _expect(t, H)
    d = th._dev(t)
    n_rec = len(t["read_id"])
    with ecb.EcBuilder(T, H) as b:
        b.push_device(*d)
        bad0, long0 = b.verify_device(*d)
        assert bad0 == 0 and long0 >= sum(n >= 1100 for n in lengths) * 5
        for r, key, n in targets:
            t2 = _swap(t, r, key)
            want = misplaced(t, t2, H)
            assert int(want.sum()) == 1 and want[r]
            d2 = [d[0], _up(t2["locus"]), _up(t2["hapflag"])]
            assert b.verify_device(*d2)[0] == 1, n
            assert b.verify_device_tiled(ecb.tile_tuples(*d2), n_rec)[0] == 1, n
        assert b.verify_device(*d) == (bad0, long0)                      # (the pass left the handle as it found it)
        _check(b.export(), b.finalize(), exp)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


# ---- merges --------------------------------------------------------------------------------------------------------------------------------
_MERGE = {}


def _merge_stream(group):
    """Two contiguous read shards.  Per key length class -- inline (2, 5), arena (6, 17), long (17 and 40: beyond RANKED_MAX) -- three
    layouts, each on an instance of its own: A only in shard 0 and B only in shard 1; both in both (in opposite orders); both in shard 0
    and neither in shard 1; and one pair of 2 100 pairs (beyond BIG_LDS; k_slow founds it) in both shards.  Some 3 000 filler ECs per
    shard, so that a root table of 1 024 slots has to grow.
    -> dict(t, exp, cut [first read of shard 1], pairs)."""
    if group in _MERGE:
        return _MERGE[group]
    rng = np.random.default_rng(31)
    fams = GROUPS[group]
    H = _H(fams[0])
    shard = [[], []]
    pairs = []
    for ni, n in enumerate((2, 5, 6, 17, 40, 2100)):
        for li in range(3):
            fam = fams[(ni + li) % len(fams)]
            if n == 2100 and li != 1:
                continue
            ka, kb = _pair(fam, 3 * ni + li, n, WHERES[(ni + li) % 3])
            pairs.append((ka, kb))
            ra, rb = sh.read_of(ka, ORDERS[li % 2]), sh.read_of(kb, ORDERS[ni % 2])
            if li == 0:
                shard[0] += [ra, ra]
                shard[1] += [rb, rb, rb]
            elif li == 1:
                shard[0] += [ra, rb, ra]
                shard[1] += [rb, ra]
            else:
                shard[0] += [rb, ra, rb]
    reads = []
    for s in (0, 1):
        fill = [th._distinct(rng, int(rng.integers(2, 9)), T, H) for _ in range(3000)]
        for r in shard[s]:
            fill.insert(int(rng.integers(0, len(fill) + 1)), r)
        shard[s] = fill
        reads += fill
    t = th._stream(reads)
    out = dict(t=t, exp=_expect(t, H), cut=len(shard[0]), pairs=pairs, H=H)
    _MERGE[group] = out
    return out


def _shard_builders(S, **kw):
    t, H = S["t"], S["H"]
    n_reads = int(t["read_id"][-1]) + 1
    cuts = [int(np.searchsorted(t["read_id"], r)) for r in (0, S["cut"], n_reads)]
    out = []
    for a, z in zip(cuts[:-1], cuts[1:]):
        b = ecb.EcBuilder(T, H, ec_capacity=1 << 10, **kw)
        b.push(t["read_id"][a:z] - t["read_id"][a], t["locus"][a:z], t["hapflag"][a:z])
        out.append(b)
    return out


def _check_root(b, S):
    s = b.sizes or b.finalize()
    _check(b.export(), s, S["exp"])
    exp = S["exp"]
    _assert_collide(_device_hashes(b), _rows_of(exp["indptr"], exp["indices"], exp["data"]), S["pairs"])


@pytest.mark.parametrize("group", ["h8", "h24"])
def test_colliding_ecs_through_the_table_merges_and_adopts(group):
    """``ListCmp::quick`` and ``ListCmp::full`` returning CMP_DIFFERENT inside ``k_merge``, and the probe-on of ``ecb.hip: k_merge`` behind
    ST_OTHER: the shards of ``_merge_stream`` (a) merged whole into a root of 1 024 slots, one ``ecb_table_merge_device`` per shard;
    (b) cut into two key ranges (a colliding pair shares its range: the range is picked by the hash), range 0 merged table by table and
    range 1 by ``ecb_table_merge_batch_device``, the parts adopted by ``ecb_table_adopt_device`` one by one and by
    ``ecb_table_adopt_batch_device`` into roots of 1 024 slots; each == one handle over the whole stream == the oracles, the colliding
    ECs apart with equal exported hashes."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    S = _merge_stream(group)
    H = S["H"]
    out, sizes = _run_host(S["t"], T, H, batch=5001)
    _check(out, sizes, S["exp"])
    _witness(S["t"], H, S["exp"], S["pairs"])
    shards = _shard_builders(S)
    meta, base, whole, pieces = [], 0, [], []
    for b in shards:
        eng = ecdist.GpuEngine(b, dev)
        ne, npairs, nreads = b.table_sizes()
        whole.append(eng.table_export(base) + (ne, npairs))
        pieces.append(eng.table_export_parts(base, 2))
        meta.append(b.counters()[:2])
        base += nreads
        b.close()
    totals = (sum(m[0] for m in meta), sum(m[1] for m in meta), base)
    # (a)
    root = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=64), dev)
    for ent, prs, ne, npairs in whole:
        root.table_merge(ent, ne, prs, npairs)
    root.add_counters(*totals)
    _check_root(root.b, S)
    root.b.close()
    # (b)
    adopted = []
    for q in range(2):
        part = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=64), dev)
        tabs = [(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q]) for ent, prs, eo, po in pieces]
        if q == 0:
            for tab in tabs:
                part.table_merge(*tab)
        else:
            part.table_merge_many(tabs)
        pe_n, pp_n, _ = part.table_sizes()
        adopted.append(part.table_export(0) + (pe_n, pp_n))
        part.b.close()
    for many in (False, True):
        root = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=64), dev)
        if many:
            root.table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
        else:
            for pe, pp, pe_n, pp_n in adopted:
                root.table_adopt(pe, pe_n, pp, pp_n)
        root.add_counters(*totals)
        _check_root(root.b, S)
        root.b.close()


@pytest.mark.parametrize("group", ["h8", "h24"])
def test_colliding_ecs_through_ecb_merge_and_the_key_range_finalize(group):
    """The same shards through ``ecb_merge`` (``EcBuilder.merge_from``: the multi-GPU merge inside the library) and through the key-range
    path of ``dist.py`` as ``test_gpu_dist.py`` drives it in one process (``table_export_parts`` -> ``table_rebase`` ->
    ``table_merge_many`` -> ``finalize_range`` -> ``assemble_ranges``; the assembled result's hashes come from ``k_row_keys``)."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    S = _merge_stream(group)
    H = S["H"]
    sh_ = _shard_builders(S)
    with ecb.EcBuilder(T, H, ec_capacity=64) as r2:
        r2.merge_from(sh_)
        _check_root(r2, S)
    for b in sh_:
        b.close()
    world, cuts, bases, base, totals = 2, [], [], 0, [0, 0, 0]
    shards = _shard_builders(S)
    for b in shards:
        eng = ecdist.GpuEngine(b, dev)
        cuts.append(eng.table_export_parts(0, world))
        bases.append(base)
        a, v, n = eng.counters()
        totals = [totals[0] + a, totals[1] + v, totals[2] + n]
        base += n
    pieces = []
    for q in range(world):
        part = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=64), dev)
        part.table_merge_many([(part.table_rebase(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], b0), eo[q + 1] - eo[q], prs[po[q]:], po[q + 1] - po[q])
                               for (ent, prs, eo, po), b0 in zip(cuts, bases) if eo[q + 1] > eo[q]])
        pieces.append(part.finalize_range(*totals))
        part.b.close()
    for b in shards:
        b.close()
    with ecb.EcBuilder(T, H, ec_capacity=64) as root:
        ecdist.GpuEngine(root, dev).assemble_ranges([p for p in pieces if p[1]], *totals)
        _check_root(root, S)


# ---- k_set_global_rank ---------------------------------------------------------------------------------------------------------------------
class _CellStream(object):
    """What ``test_gpu_multisample._sharded`` needs of a stream: tuples, a cell and a file per read."""

    def __init__(self, t, cell, fil, n_loci):
        self.read_id, self.locus, self.hapflag = t["read_id"], t["locus"], t["hapflag"]
        self.cell, self.file = np.asarray(cell, np.int64), np.asarray(fil, np.int64)
        self.meta = (self.cell | (self.file << tm.CELL_BITS)).astype(np.uint32)
        self.n_reads, self.n_loci = len(cell), n_loci

    def records(self, r0, r1):
        a, b = np.searchsorted(self.read_id, [r0, r1])
        return self.read_id[a:b] - np.uint32(r0), self.locus[a:b], self.hapflag[a:b]


def test_a_shard_finds_both_ecs_of_one_hash_for_its_triples(monkeypatch):
    """``k_set_global_rank`` finds a shard's EC in the merged result "by its hash and then by its key": two of the shard's ECs share the
    hash (both keys in one shard), or the shard holds one of them and must pass the other's row over.  The multisample shard path
    (``export_ec_keys_device`` -> ``ms_local_triples_device`` -> ``ms_adopt_triples_device``, as ``test_gpu_multisample._sharded`` runs
    it) over the shards of ``_merge_stream``, the reads of the colliding keys in cells of their own: every (EC, cell, file) triple of the
    root carries its own EC's rank, count and first read -- expected from the oracles' EC order and a dict over the reads' own sets --
    and ``ms_filter`` == ``ms_checker``."""
    S = _merge_stream("h8")
    t, exp, H = S["t"], S["exp"], S["H"]
    monkeypatch.setattr(tm, "H", H)
    rows = _rows_of(exp["indptr"], exp["indices"], exp["data"])
    lens = np.bincount(t["read_id"].astype(np.int64))
    starts = np.cumsum(lens) - lens
    n_reads = len(lens)
    ec = np.empty(n_reads, np.int64)
    hap = (t["hapflag"].astype(np.int64) >> 16) & 0xFF
    for r in range(n_reads):
        d = {}
        for l, h in zip(t["locus"][starts[r]:starts[r] + lens[r]].tolist(), hap[starts[r]:starts[r] + lens[r]].tolist()):
            d[l] = d.get(l, 0) | (1 << h)
        ec[r] = rows[tuple(sorted(d.items()))]
    special = {rows[_row(k)] for p in S["pairs"] for k in p}
    n_cells = 64
    cell = np.where(np.isin(ec, list(special)), 32 + ec % 29, np.arange(n_reads) % 31)      # (the colliding keys' reads in cells 32 ..: A and B mostly apart)
    fil = (np.arange(n_reads) >= S["cut"]).astype(np.int64)
    st = _CellStream(t, cell, fil, T)
    key = (ec << 32) | (st.cell << 10) | st.file
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    k = ks[heads]
    tr = dict(ec=k >> 32, cell=(k >> 10) & (tm.MAX_CELLS - 1), file=k & 1023, count=np.diff(np.concatenate((heads, [len(ks)]))), first=order[heads])
    root, shards = tm._sharded(st, [0, S["cut"], n_reads])
    try:
        got = root.b.export_pairs()
        for name in ("ec", "cell", "file", "count", "first"):
            assert np.array_equal(got[name], tr[name]), name
        a = root.b.export()
        assert np.array_equal(a["indptrA"], exp["indptr"]) and np.array_equal(a["indicesA"], exp["indices"]) and np.array_equal(a["dataA"], exp["data"])
        _assert_collide(_device_hashes(root.b), rows, S["pairs"])
        for mc in (-1, 40):
            tm._check_filter(root.b, a, tr, len(exp["count"]), n_cells, mc)
    finally:
        root.b.close()
        for b in shards:
            b.close()


# ---- row merges without a handle -----------------------------------------------------------------------------------------------------------
def _names(n, p):
    return ["%s%06d" % (p, i) for i in range(n)]


def test_colliding_rows_through_ecmerge():
    """``ecb_combine`` puts every row of every part through ``k_cb_entries`` -> ``k_merge`` (``ListCmp``) and finds it again in
    ``k_cb_lookup`` (hash, then size, then pair for pair: ``ecb.hip: k_cb_lookup``): colliding rows of all three families (24 haplotypes),
    2 .. 2 100 pairs, within one part and across parts, each several times with counts, against ``ec_merge_checker``; the merged rows'
    numpy hashes collide (tied to the device by ``test_the_numpy_hash_is_the_device_hash``).  The parts number their columns 0 .. over
    the loci in use and reach the keys' real loci -- which the hash is taken over -- through their target maps; the checker merges the
    parts in their own numbering, which the (ascending) map carries over.

    ``ecb_salmon_ecs`` is not a caller: it writes one row per EC line in line order (``ecb.hip: k_sl_rowptr``,
    ``indptr[r] = pos[lower_bound_u64(keys, n, r << 32)]``), merges no equal rows and never hashes one."""
    from alntools_amd import bin_utils
    rng = np.random.default_rng(41)
    H = 24
    pairs, a_keys, b_keys = [], [], []
    for k, (fam, n) in enumerate((f, n) for f in ("F2", "M2", "N23") for n in (2, 5, 6, 17, 2100)):
        ka, kb = _pair(fam, 2 + k, n, WHERES[k % 3])
        pairs.append((ka, kb))
        if k % 3 == 0:                                                   # within one part | across parts | both
            a_keys += [ka, kb, ka]
        elif k % 3 == 1:
            a_keys += [ka]
            b_keys += [kb, kb]
        else:
            a_keys += [kb, ka]
            b_keys += [ka, kb, kb]
    fill = []
    for _ in range(400):
        n = int(rng.integers(1, 9))
        fill.append((np.sort(rng.choice(T, size=n, replace=False)), rng.integers(1, 1 << H, n)))
    a_keys = [a_keys[i] for i in rng.permutation(len(a_keys))] + fill[:250]
    b_keys = fill[200:] + [b_keys[i] for i in rng.permutation(len(b_keys))]
    U = np.unique(np.concatenate([k[0] for k in a_keys + b_keys]))
    lname, hname = _names(len(U), "t"), _names(H, "h")
    a_rows, b_rows = ([(np.searchsorted(U, k[0]), k[1]) for k in keys] for keys in (a_keys, b_keys))
    a = th._bin(a_rows, lname, hname, ["s1"], [{k: k + 1 for k in range(len(a_rows))}])
    b = th._bin(b_rows, lname, hname, ["s1", "s2"], [{k: 2 for k in range(0, len(b_rows), 2)}, {k: 3 for k in range(len(b_rows))}])
    for ms in ([a, b], [b, a], [a]):
        want = chk.merge(ms)
        plan = bin_utils.plan_merge(ms)
        parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                      n_loci=m.num_loci, target_map=U, sample_map=sm) for m, sm in zip(ms, plan.sample_maps)]
        got = ecb.combine(parts, T, H, len(plan.sname))
        assert plan.sname == want.sname
        for g, name in zip(got, ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")):
            w = np.asarray(getattr(want, name), np.int64)
            assert np.array_equal(np.asarray(g, np.int64), U[w] if name == "indicesA" else w), name
        ip, ix, da = (np.asarray(g, np.int64) for g in got[:3])
        rows = _rows_of(ip, ix, da)
        here = [p for p in pairs if _row(p[0]) in rows and _row(p[1]) in rows]
        assert len(here) == (len(pairs) if len(ms) == 2 else 2 * len(pairs) // 3)
        _assert_collide(sh.row_hashes(ip, ix, da), rows, here)


def test_colliding_rows_through_ecbundle():
    """``ecb_bundle`` folds the bundled rows through the same ``k_cb_entries`` -> ``k_merge`` -> ``k_cb_lookup``: a grouping under which
    the BUNDLED rows are the colliding keys -- input loci 2 i and 2 i + 1 both belong to group U[i], U the loci of the keys, and a row
    holds a pair's mask whole on locus 2 i or split over the two -- so rows that differ before the bundle fold into the two ECs of one
    hash (F2 and N23, 8 haplotypes; 2 .. 2 100 pairs), against ``bundle_checker`` (which numbers the groups in use 0 .. ; the ascending
    map U carries its columns over to the group ids the device hashed)."""
    rng = np.random.default_rng(43)
    H = 8
    keys, pairs = [], []
    for k, (fam, n) in enumerate((f, n) for f in ("F2", "N23") for n in (2, 5, 6, 17, 2100)):
        ka, kb = _pair(fam, 4 + k, n, WHERES[k % 3])
        pairs.append((ka, kb))
        keys += [ka, kb]
    for _ in range(200):
        n = int(rng.integers(1, 9))
        keys.append((np.sort(rng.choice(T, size=n, replace=False)), rng.integers(1, 1 << H, n)))
    U = np.unique(np.concatenate([k[0] for k in keys]))
    small = [[2 * i, 2 * i + 1] for i in range(len(U))]                   # the checker's groups: those in use
    groups = [[] for _ in range(T)]                                      # the device's: group U[i] of T
    for i, g in enumerate(U.tolist()):
        groups[g] = small[i]

    def row(key, split):
        cols, masks = [], []
        for l, m in zip(key[0].tolist(), key[1].tolist()):
            i = int(np.searchsorted(U, l))
            low = m & -m
            if split and m != low:
                cols += [2 * i, 2 * i + 1]
                masks += [low, m ^ low]
            else:
                cols.append(2 * i + (l % 2 if split else 0))
                masks.append(m)
        return np.array(cols, np.int64), np.array(masks, np.int64)
    rows_in = [row(k, s) for k in keys for s in (False, True)] + [row(k, True) for k in keys[:len(pairs) * 2]]
    rows_in = [rows_in[i] for i in rng.permutation(len(rows_in))]
    m = th._bin(rows_in, _names(2 * len(U), "t"), _names(H, "h"), ["s1", "s2"],
                [{k: 1 + k % 5 for k in range(len(rows_in))}, {k: 2 for k in range(0, len(rows_in), 3)}])
    ptr, idx = bchk.group_csr(m.num_loci, groups)
    got = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, m.num_loci, H, T, ptr, idx)
    want = bchk.bundle(m, _names(len(U), "g"), small)
    for g, name in zip(got, ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")):
        w = np.asarray(getattr(want, name), np.int64)
        assert np.array_equal(np.asarray(g, np.int64), U[w] if name == "indicesA" else w), name
    ip, ix, da = (np.asarray(g, np.int64) for g in got[:3])
    assert len(ip) - 1 == len(keys)                                      # every key one EC, the split and the whole rows folded together
    _assert_collide(sh.row_hashes(ip, ix, da), _rows_of(ip, ix, da), pairs)
