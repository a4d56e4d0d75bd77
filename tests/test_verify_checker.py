"""``verify_checker.misplaced`` -- the expected count of every exactness-pass test -- pinned on hand-written reads, one for every way two
target sets can differ and two where records change but the set does not, and checked on random reads against a second opinion: the C
oracle over read r of the pushed stream followed by read r of the changed one (the stream ``t`` followed by ``t2`` with its read ids moved
on by the number of reads, one read at a time, since the oracle returns counts and no per-read ids): the two fall into different ECs iff
the oracle counts two ECs.  ``verify_checker.perturb`` -- the changes the GPU tests make -- is held to the tuple contract here."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import ec_oracle as orc

from verify_checker import COUNTED, KINDS, NOT_COUNTED, misplaced, perturb

H = 4
INV = 0x4


def _t(reads):
    """reads: lists of (locus, hap, flag) records -> tuple dict."""
    rid = np.array([k for k, r in enumerate(reads) for _ in r], np.uint32)
    loc = np.array([x[0] for r in reads for x in r], np.uint32)
    hf = np.array([x[2] | (x[1] << 16) for r in reads for x in r], np.uint32)
    return dict(read_id=rid, locus=loc, hapflag=hf)


BASE = [(10, 0, 0), (11, 1, 0), (12, 2, INV), (13, 3, 0), (14, 0, 0), (15, 1, 0), (16, 2, 0)]     # sets: 10:1 11:2 13:8 14:1 15:2 16:4
OTHER = [(7, 1, 0), (8, 1, INV)]
HAND = {
    # kind -> (read 1 as changed, misplaced)
    "hap": ([(10, 0, 0), (11, 3, 0)] + BASE[2:], True),
    "locus": ([(10, 0, 0), (99, 1, 0)] + BASE[2:], True),
    "drop": (BASE[:3] + [(13, 3, INV)] + BASE[4:], True),
    "new_locus": (BASE[:2] + [(17, 2, 0)] + BASE[3:], True),
    "new_bit": (BASE[:2] + [(14, 2, 0)] + BASE[3:], True),
    "hap_highest": (BASE[:6] + [(16, 0, 0)], True),
    "hap_lowest": ([(10, 1, 0)] + BASE[1:], True),
    "permute": (BASE[:1] + BASE[:0:-1], False),
    "dup": (BASE[:2] + [(15, 1, 0)] + BASE[3:], False),
    # records change, the set does not: an invalid record moves to another locus and haplotype; a valid record is doubled
    "invalid_moved": (BASE[:2] + [(500, 0, INV)] + BASE[3:], False),
    "invalid_made_valid_copy_of_head": (BASE[:2] + [(10, 0, 0)] + BASE[3:], False),
    # ... and the paired-end filter: a record that fails it as a mate on another reference counts as little as an unmapped one
    "valid_becomes_mate_elsewhere": (BASE[:3] + [(13, 3, 0x1 | 0x2 | 0x1000)] + BASE[4:], True),
    "valid_becomes_proper_pair": (BASE[:3] + [(13, 3, 0x1 | 0x2 | 0x40)] + BASE[4:], False),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_reads(name):
    changed, want = HAND[name]
    t, t2 = _t([OTHER, BASE, OTHER]), _t([OTHER, changed, OTHER])
    assert len(changed) == len(BASE) and not (np.array_equal(t["locus"], t2["locus"]) and np.array_equal(t["hapflag"], t2["hapflag"]))
    assert misplaced(t, t2, H).tolist() == [False, want, False]
    assert misplaced(t2, t, H).tolist() == [False, want, False]
    assert not misplaced(t, t, H).any()


def test_every_kind_has_a_hand_written_read_and_perturb_makes_that_change():
    assert set(KINDS) <= set(HAND) and set(COUNTED) | set(NOT_COUNTED) == set(KINDS)
    t = _t([OTHER, BASE, OTHER])
    for kind in KINDS:
        t2 = perturb(t, 1, kind, 1000, H)
        assert t2 is not None and t2["read_id"] is t["read_id"], kind
        assert misplaced(t, t2, H).tolist() == [False, kind in COUNTED, False], kind
        want = _t([OTHER, HAND[kind][0], OTHER])
        if kind not in ("locus", "new_locus", "new_bit", "hap", "drop", "dup"):      # (these pick their record or value by a rule of their own)
            assert np.array_equal(t2["locus"], want["locus"]) and np.array_equal(t2["hapflag"], want["hapflag"]), kind
    # what a read has not got the records for is refused, not faked
    one = _t([[(5, 0, 0)]])
    assert [k for k in KINDS if perturb(one, 0, k, 1000, H) is not None] == ["hap", "locus", "hap_highest", "hap_lowest"]
    two_valid = _t([[(5, 0, 0), (6, 1, 0)]])
    assert perturb(two_valid, 0, "permute", 1000, H) is None and perturb(two_valid, 0, "dup", 1000, H) is None


def _pair_says_different(t, t2, r):
    """The C oracle over read r of ``t`` then read r of ``t2``: two ECs iff the sets differ."""
    a, z = np.searchsorted(t["read_id"], [r, r + 1])
    rid = np.concatenate([np.zeros(z - a, np.uint32), np.ones(z - a, np.uint32)])
    exp = c_oracle.ec_from_tuples(rid, np.concatenate([t["locus"][a:z], t2["locus"][a:z]]),
                                  np.concatenate([t["hapflag"][a:z], t2["hapflag"][a:z]]), H)
    assert exp["n_reads"] == 2 and int(exp["count"].sum()) == 2
    return len(exp["count"]) == 2


def _random_reads(rng, n, T):
    """Reads of 1 .. 12 records on few loci (loci and (locus, haplotype) pairs repeat within a read), a fifth of the records behind the
    head invalid by one of the filter's bits."""
    reads = []
    for _ in range(n):
        k = int(rng.integers(1, 13))
        base = int(rng.integers(0, T - 8))
        flags = rng.choice([0, 0, 0, 0, INV, 0x1 | 0x2 | 0x40, 0x1 | 0x40, 0x1 | 0x2 | 0x80], size=k)
        flags[0] = 0
        reads.append(list(zip((base + rng.integers(0, 8, k)).tolist(), rng.integers(0, H, k).tolist(), flags.tolist())))
    return reads


@pytest.mark.parametrize("seed", [0, 1])
def test_checker_agrees_with_the_c_oracle_on_random_reads(seed):
    rng = np.random.default_rng(seed)
    T, R = 60, 300
    t = _t(_random_reads(rng, R, T))
    # every read changed: by one of the kinds, or (every third) by redrawing the records behind its head altogether
    t2 = dict(t, locus=t["locus"].copy(), hapflag=t["hapflag"].copy())
    kinds_made = set()
    for r in range(R):
        a, z = np.searchsorted(t["read_id"], [r, r + 1])
        if r % 3 == 0:
            k = z - a - 1
            t2["locus"][a + 1:z] = t["locus"][a] + rng.integers(0, 3, k)
            t2["hapflag"][a + 1:z] = (rng.integers(0, H, k) << 16) | rng.choice([0, 0, INV], size=k)
            continue
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        p = perturb(t, r, kind, T, H)
        if p is not None:
            kinds_made.add(kind)
            t2["locus"][a:z], t2["hapflag"][a:z] = p["locus"][a:z], p["hapflag"][a:z]
            assert int(p["locus"].max()) < T and orc.tuples_valid(p["hapflag"][a:a + 1])[0] and int((p["hapflag"] >> 16).max()) < H
            assert bool(misplaced(t, p, H)[r]) == (kind in COUNTED) and int(misplaced(t, p, H).sum()) <= 1, (r, kind)
    assert kinds_made == set(KINDS)
    got = misplaced(t, t2, H)
    want = np.array([_pair_says_different(t, t2, r) for r in range(R)])
    assert np.array_equal(got, want)
    assert 0 < got.sum() < R and (~got[::3]).any() and got[::3].any()
    # ... and the whole stream followed by the changed one, read ids moved on: as many reads, and no fewer ECs than either half
    both = c_oracle.ec_from_tuples(np.concatenate([t["read_id"], t["read_id"] + np.uint32(R)]), np.concatenate([t["locus"], t2["locus"]]),
                                   np.concatenate([t["hapflag"], t2["hapflag"]]), H)
    assert both["n_reads"] == 2 * R
