"""The flush of the stream kernel (``alntools_amd/csrc/k_stream.inc``, phase (c)) looks its reads up in explicit trips to the EC table: in a
trip every unsettled lane has its operation in flight -- the loads of the line it looks at, or the compare-and-swap on the slot it found
empty -- and the wave waits once.  The streams here are shaped so that the lanes of one flush are in every state at once: long probe chains
with founders among them, the same new EC twice in one pass next to a read whose hash meets the same slot, a table that fills up and grows in
mid-stream, batches that end inside reads, reads whose key is longer than a slot holds, passes in which every read founds an EC.

Every case runs under the three compilations of the kernel (``ks_std``, ``ks_short``, ``ks_par``: the library reads ``ECB_FORCE_SHORT`` /
``ECB_FORCE_PAR`` when it picks one) and holds CSR A, N and the three counters to ``oracle/ec_oracle.c`` bit for bit; the exactness pass
(``verify_device``) must then find 0 reads whose target set differs from their EC's key.

Streams: a few thousand reads of 1 - 3 records over 64 loci and 2 haplotypes -- a 512-record tile then holds more reads than a pass takes
(64, or 128 in ``ks_short``), so every pass is full -- into the smallest table the builder makes (1024 slots)."""
import itertools

import numpy as np
import pytest

from alntools_amd import ecb
from set_hash import set_hash

gpu = pytest.mark.gpu

T, H = 64, 2
CAP = 1024                      # the smallest EC table (ecb_create rounds ec_capacity up to it)
VARIANTS = [("ks_std", None), ("ks_short", "ECB_FORCE_SHORT"), ("ks_par", "ECB_FORCE_PAR")]


# ---- keys and streams ------------------------------------------------------------------------------------------------------------------
def _key_pool():
    """Every key {locus -> mask} over 64 loci and 2 haplotypes that 1 - 3 records spell: (loci, masks) tuples, in a fixed order."""
    pool = [((l,), (m,)) for l in range(T) for m in (1, 2, 3)]
    for a, b in itertools.combinations(range(T), 2):
        pool += [((a, b), ms) for ms in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (1, 3), (2, 3))]
    for a, b, c in itertools.combinations(range(0, T, 3), 3):
        pool += [((a, b, c), ms) for ms in itertools.product((1, 2), repeat=3)]
    return pool


_POOL = _key_pool()
_HASH = {}


def _hash(key):
    if key not in _HASH:
        _HASH[key] = set_hash(np.array(key[0]), np.array(key[1]))
    return _HASH[key]


def _records(key, rng=None):
    """The records of one read whose target set is `key`: one per set haplotype bit, the loci in a shuffled order when `rng` is given."""
    recs = [(l, h) for l, m in zip(*key) for h in range(H) if m >> h & 1]
    if rng is not None:
        rng.shuffle(recs)
    return recs


def _stream(keys, rng=None):
    """Tuple streams of the reads `keys` (one read per key, in order): single-end records, all valid."""
    rid, loc, hf = [], [], []
    for r, k in enumerate(keys):
        for l, h in _records(k, rng):
            rid.append(r)
            loc.append(l)
            hf.append(h << 16)
    return dict(read_id=np.array(rid, np.uint32), locus=np.array(loc, np.uint32), hapflag=np.array(hf, np.uint32), n_reads=len(keys))


def _probe_lengths(keys, cap=CAP):
    """Linear probing from hash & (cap - 1), the keys inserted in the order they first appear -- the rule of the kernel's table, without the
    races: per read the number of slots its lookup looks at, and whether it ends on an empty slot (a founder)."""
    slots, out = {}, []
    for k in keys:
        h = _hash(k)
        j, n = h & (cap - 1), 1
        while j in slots and slots[j] != k:
            j, n = (j + 1) & (cap - 1), n + 1
        out.append((n, j not in slots))
        slots[j] = k
    return out, len(slots)


def _long_chains():
    """717 distinct ECs into 1024 slots (load 0.70), one read each, then 2 300 reads that look them up again: most passes have a lane that
    looks at four slots or more, and founders that find their first slot taken claim at the second or later."""
    rng = np.random.default_rng(11)
    ecs = [_POOL[i] for i in rng.choice(len(_POOL), 717, replace=False)]
    keys = ecs[:400] + [ecs[i] for i in rng.integers(0, 400, 300)] + ecs[400:] + [ecs[i] for i in rng.integers(0, 717, 2000)]
    return _stream(keys, rng), keys


def _twice_next_to_a_collider():
    """Triples A, C, A in one pass: A a new EC, C a new EC whose hash meets the same slot of the 1024 -- the second A finds the slot claimed with
    its own hash by a lane of its own wave (or loses the claim to it) and waits for that lane's key; C probes on behind both."""
    by_slot = {}
    for k in _POOL[:6000]:
        by_slot.setdefault(_hash(k) & (CAP - 1), []).append(k)
    pairs = [v[:2] for v in by_slot.values() if len(v) >= 2]
    assert len(pairs) >= 250
    keys = []
    for a, c in pairs[:250]:
        keys += [a, c, a]
    keys += [keys[i] for i in np.random.default_rng(5).integers(0, len(keys), 1250)]
    return _stream(keys), keys


def _growth():
    """3 000 distinct ECs among 4 000 reads into 1024 slots, in one push: lookups run out of probes, the wave parks, the host grows the table
    x 4 (to 4096: load 0.73) and the kernel takes every slice up where its pass began."""
    rng = np.random.default_rng(23)
    ecs = [_POOL[i] for i in rng.choice(len(_POOL), 3000, replace=False)]
    keys = list(ecs)
    for i in rng.integers(0, 3000, 1000):
        keys.insert(int(rng.integers(0, len(keys))), ecs[i])
    return _stream(keys, rng), keys


def _long_keys():
    """Reads of 8 loci -- more than the five pairs a slot holds, the rest in the key arena -- founded and looked up again among short reads at a
    load of 0.7."""
    rng = np.random.default_rng(31)
    ecs = [_POOL[i] for i in rng.choice(len(_POOL), 640, replace=False)]
    longs = []
    for i in range(77):
        loci = tuple(sorted(rng.choice(T, 8, replace=False).tolist()))
        longs.append((loci, tuple(int(m) for m in rng.integers(1, 3, 8))))
    longs = list(dict.fromkeys(longs))
    keys = []
    for i, k in enumerate(ecs):
        keys.append(k)
        if i % 8 == 3:
            keys.append(longs[(i // 8) % len(longs)])
    keys += [(ecs + longs)[i] for i in rng.integers(0, len(ecs) + len(longs), 1800)]
    return _stream(keys, rng), keys


def _all_new():
    """780 reads, every one a new EC, into 1024 slots: no lane of any pass is settled by its first trip."""
    rng = np.random.default_rng(47)
    keys = [_POOL[i] for i in rng.choice(len(_POOL), 780, replace=False)]
    return _stream(keys, rng), keys


_CASES = {"long_chains": _long_chains, "twice_next_to_a_collider": _twice_next_to_a_collider, "growth": _growth, "long_keys": _long_keys,
          "all_new": _all_new}
_made, _expected = {}, {}


def _case(name, oracle=True):
    """(streams, keys, the oracle's result) of a case: made once, shared, never changed."""
    if name not in _made:
        t, keys = _CASES[name]()
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _made[name] = (t, keys)
    if oracle and name not in _expected:
        from oracle import c_oracle
        t = _made[name][0]
        _expected[name] = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=1)
    return _made[name] + (_expected.get(name),)


# ---- running ---------------------------------------------------------------------------------------------------------------------------
def _check(out, sizes, exp):
    assert (sizes["all_alignments"], sizes["valid_alignments"], sizes["n_reads"]) == (exp["n_all"], exp["n_valid"], exp["n_reads"])
    assert sizes["n_ecs"] == len(exp["count"])
    for a, k in (("indptrA", "indptr"), ("indicesA", "indices"), ("dataA", "data"), ("dataN", "count")):
        assert np.array_equal(out[a], exp[k]), a
    assert out["indptrN"].tolist() == [0, len(exp["count"])]
    assert np.array_equal(out["indicesN"], np.arange(len(exp["count"])))


def _force(monkeypatch, env):
    for k in ("ECB_FORCE_SHORT", "ECB_FORCE_PAR", "ECB_NO_SHORT", "ECB_NO_PAR"):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, "1")


def _run(t, exp, kernel, env, monkeypatch, batch=None):
    import torch
    _force(monkeypatch, env)
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(t[k].view(np.int32).copy()).to(dev) for k in ("read_id", "locus", "hapflag")]
    with ecb.EcBuilder(T, H, ec_capacity=CAP) as b:
        # (the kernel for short reads is only taken for a stream whose number of reads is known; with the number known and fewer than seven
        #  records per read the library takes it by itself, so the other two run without)
        b.hint_reads(t["n_reads"] if kernel == "ks_short" else 0)
        if batch:
            for a in range(0, len(t["read_id"]), batch):
                b.push(t["read_id"][a:a + batch], t["locus"][a:a + batch], t["hapflag"][a:a + batch])
        else:
            b.push_device(*d)
        # (with neither variable set the choice is the library's: it takes ks_par for the batches behind one in which more than a quarter of
        #  the tiles had records whose first place in the pass's table was taken)
        assert b.profile_kernel().startswith((kernel + "::",) + (("ks_par::",) if batch and not env else ())), b.profile_kernel()
        s = b.finalize()
        _check(b.export(), s, exp)
        b.reset()
        b.push_device(*d)
        assert b.verify_device(*d) == (0, 0)


def _assert_long_chain_shape():
    """By the table's own rule at least a tenth of the 64-read passes hold a read that looks at four slots or more, and founders are
    displaced onto empty slots (their claim is made at the second probe or later)."""
    t, keys, _ = _case("long_chains", oracle=False)
    pl, used = _probe_lengths(keys)
    assert used == 717 and 0.69 < used / CAP < 0.71
    passes = [pl[a:a + 64] for a in range(0, len(pl), 64)]
    deep = sum(1 for p in passes if max(n for n, _ in p) >= 4)
    print("passes with a lookup of 4+ slots: %d of %d; displaced founders: %d" % (deep, len(passes), sum(1 for n, f in pl if f and n >= 2)))
    assert deep * 10 >= len(passes)
    assert any(f and n >= 2 for n, f in pl)
    assert max(n for n, _ in pl) < 256                      # (no lookup runs out of probes: the table does not grow)
    rec = np.bincount(t["read_id"])
    assert rec.min() >= 1 and rec.max() <= 3


def test_the_long_chain_stream_has_the_shape_it_is_meant_to_have():
    """(needs no GPU: the stream is judged with the hash restated in tests/set_hash.py)"""
    _assert_long_chain_shape()


@gpu
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_long_chains_with_founders_among_them(kernel, env, monkeypatch):
    _assert_long_chain_shape()                              # before the GPU is touched
    t, _, exp = _case("long_chains")
    assert len(exp["count"]) == 717
    _run(t, exp, kernel, env, monkeypatch)


@gpu
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_the_same_new_ec_twice_in_one_pass_next_to_a_collider(kernel, env, monkeypatch):
    t, keys, exp = _case("twice_next_to_a_collider")
    for a, c, a2 in (keys[0:3], keys[300:303], keys[747:750]):      # (the stream is what it says: A, C, A with A and C on one slot)
        assert a == a2 and a != c and _hash(a) != _hash(c) and (_hash(a) ^ _hash(c)) & (CAP - 1) == 0
    _run(t, exp, kernel, env, monkeypatch)


@gpu
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_the_table_fills_up_and_grows_in_mid_stream(kernel, env, monkeypatch):
    t, keys, exp = _case("growth")
    assert len(exp["count"]) == 3000 > CAP                  # (more ECs than slots: the push cannot end without a park and a larger table)
    _run(t, exp, kernel, env, monkeypatch)


@gpu
@pytest.mark.parametrize("batch", [1, 7, 1000, 4097])
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_batches_that_end_inside_reads(kernel, env, batch, monkeypatch):
    t, _, exp = _case("long_chains")
    n = 1500 if batch == 1 else len(t["read_id"])           # (a launch per record: the first 1 500 records, cut on a read boundary)
    while batch == 1 and t["read_id"][n] == t["read_id"][n - 1]:
        n += 1
    if n < len(t["read_id"]):
        from oracle import c_oracle
        t = dict({k: t[k][:n] for k in ("read_id", "locus", "hapflag")}, n_reads=int(t["read_id"][n - 1]) + 1)
        exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=1)
    assert batch == 4097 or any(t["read_id"][a] == t["read_id"][a - 1] for a in range(batch, len(t["read_id"]), batch))
    _run(t, exp, kernel, env, monkeypatch, batch=batch)


@gpu
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_reads_with_more_loci_than_a_slot_holds_among_the_unsettled(kernel, env, monkeypatch):
    t, keys, exp = _case("long_keys")
    assert sum(1 for k in keys if len(k[0]) == 8) >= 150 and max(np.diff(exp["indptr"])) == 8
    _run(t, exp, kernel, env, monkeypatch)


@gpu
@pytest.mark.parametrize("kernel,env", VARIANTS)
def test_passes_in_which_every_read_founds_an_ec(kernel, env, monkeypatch):
    t, keys, exp = _case("all_new")
    assert len(exp["count"]) == len(keys) == 780
    _run(t, exp, kernel, env, monkeypatch)
