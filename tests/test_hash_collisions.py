"""The committed collisions of the EC table's set hash (``tests/golden/hash_collisions.json``, made by ``tests/golden/make_hash_collisions.py``)
are what ``test_gpu_hash_collisions.py`` stands on: every one of them, at every padded length that file uses, must be two DIFFERENT valid
keys with EQUAL hashes under the numpy restatement ``set_hash.py`` -- and the restatement's constants must be the ones in
``alntools_amd/csrc/ecb.hip``.  A retune of the hash fails here first: regenerate the fixture with ``make_hash_collisions.py`` (minutes
of one CPU core) and restate the new hash in ``set_hash.py``."""
import os
import re

import numpy as np
import pytest

import set_hash as sh

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")
FX = sh.load()
#: every (length of key a, place of the differing pairs) test_gpu_hash_collisions.py pads to
LENGTHS = (2, 5, 6, 9, 10, 17, 40, 65, 81, 1100, 2100)
WHERE = ("low", "mid", "high")
REGEN = "the set hash changed: restate it in tests/set_hash.py and regenerate tests/golden/hash_collisions.json with tests/golden/make_hash_collisions.py"


def _cases():
    return [(f, i) for f in ("F2", "M2", "N23") for i in range(len(FX["families"][f]["collisions"]))]


def test_the_fixture_holds_several_instances_of_every_family():
    assert set(FX["families"]) == {"F2", "M2", "N23"}
    for f, d in FX["families"].items():
        assert len(d["collisions"]) >= 4, f
    assert FX["families"]["F2"]["n_haps"] == 8 and FX["families"]["N23"]["n_haps"] == 8 and FX["families"]["M2"]["n_haps"] == 24
    (l0, l1), (h0, h1) = FX["pad_low"], FX["pad_high"]
    assert 0 < l0 < l1 <= h0 < h1 <= FX["n_loci"]


@pytest.mark.parametrize("family,i", _cases(), ids=["%s-%d" % c for c in _cases()])
def test_every_collision_at_every_padded_length(family, i):
    fam = FX["families"][family]
    c, H = fam["collisions"][i], fam["n_haps"]
    a, b = c["a"], c["b"]
    assert len(a) == 2 and len(b) == (3 if family == "N23" else 2)
    if family == "F2":
        assert len({p[0] for p in a + b}) == 4                             # four different loci
    if family == "M2":
        assert [p[0] for p in a] == [p[0] for p in b] and all(x[1] != y[1] for x, y in zip(a, b))     # the same two loci, other masks
    (l0, l1), (h0, h1) = FX["pad_low"], FX["pad_high"]
    for p in a + b:
        assert l1 <= p[0] < h0, "a differing locus inside a padding range"
    for n in LENGTHS:
        for where in WHERE:
            ka, kb = sh.pad(c, n, where, FX)
            assert len(ka[0]) == n and len(kb[0]) == n + (family == "N23")
            for loci, masks in (ka, kb):
                assert np.all(np.diff(loci) > 0)                           # distinct within a key (and sorted)
                assert loci.min() >= 0 and loci.max() < FX["n_loci"]
                assert masks.min() >= 1 and masks.max() < (1 << H)
            assert sorted(zip(ka[0].tolist(), ka[1].tolist())) != sorted(zip(kb[0].tolist(), kb[1].tolist()))
            ha, hb = sh.set_hash(*ka), sh.set_hash(*kb)
            assert ha == hb, (family, i, n, where)
            if n == 2:
                assert ha == int(c["hash"], 16)
            # where the differing pairs sit: below, among or above the padding
            diff_a = np.flatnonzero(~np.isin(ka[0], kb[0]) | (ka[1] != kb[1][np.searchsorted(kb[0], ka[0]).clip(0, len(kb[0]) - 1)]))
            assert len(diff_a) == 2
            if n > 3:
                assert {"low": diff_a.max() == 1, "high": diff_a.min() == n - 2, "mid": 0 < diff_a.min() and diff_a.max() < n - 1}[where]


def test_reads_of_a_key_hold_the_key():
    c = FX["families"]["M2"]["collisions"][0]
    for order in ("asc", "desc"):
        for key in sh.pad(c, 6, "mid", FX):
            loci, haps = sh.read_of(key, order)
            got = {}
            for l, h in zip(loci.tolist(), haps.tolist()):
                got[l] = got.get(l, 0) | (1 << h)
            assert got == dict(zip(key[0].tolist(), key[1].tolist()))
            assert (np.diff(loci) >= 0).all() if order == "asc" else (np.diff(loci) <= 0).all()


def test_known_values():
    """A collision found by an independent search before this restatement was written (its pair sums are 0xe63b7244e6800001 with bit 0
    set; finish_hash adds 2 x (2^32 + 1) for the two pairs), and the empty key."""
    h = (0xe63b7244e6800001 + 2 * sh.N_TERM) | 1
    assert sh.set_hash([17016, 55842], [238, 136]) == sh.set_hash([97611, 115741], [231, 61]) == h
    assert sh.set_hash([], []) == 1
    assert sh.row_hashes([0, 2, 2, 4], [17016, 55842, 97611, 115741], [238, 136, 231, 61]).tolist() == [h, 1, h]


# ---- the constants, against the kernel source ------------------------------------------------------------------------------------------------
def _source():
    with open(os.path.join(CSRC, "ecb.hip")) as f:
        return f.read()


PINNED = [
    (r"h \^= h >> 16; h \*= 0x%08XU;" % sh.FMIX_MUL1, "fmix32: first shift and multiplier"),
    (r"h \^= h >> 13; h \*= 0x%08XU;" % sh.FMIX_MUL2, "fmix32: second shift and multiplier"),
    (r"h \*= 0x%08XU;\s*\n\s*h \^= h >> 16;\s*\n\s*return h;" % sh.FMIX_MUL2, "fmix32: last shift"),
    (r"const u32 h0 = fmix32\(locus \* 0x%08XU \+ mask \* 0x%08XU \+ 0x%08XU\);" % (sh.MUL_LOCUS, sh.MUL_MASK, sh.ADD0), "pair_hash64: low word"),
    (r"const u32 h1 = fmix32\(\(h0 \^ locus\) \* 0x%08XU \+ mask\);" % sh.MUL_H1, "pair_hash64: high word"),
    (r"return \(\(u64\)h1 << 32\) \| h0;", "pair_hash64: the two words"),
    (r"u64 finish_hash\(u64 s0, u32 n\) \{ return \(s0 \+ \(\(u64\)n << 32\) \+ n\) \| 1ull; \}", "finish_hash"),
]


@pytest.mark.parametrize("pattern,what", PINNED, ids=[p[1] for p in PINNED])
def test_hash_constants_are_those_of_the_kernel_source(pattern, what):
    assert len(re.findall(pattern, _source(), re.I)) == 1, "%s: %s" % (what, REGEN)


def test_every_kernel_hashes_through_the_one_pair_hash():
    """No second mix anywhere: whatever sums a key's hash calls pair_hash64 and closes with finish_hash."""
    src = _source()
    assert len(re.findall(r"u64 pair_hash64\(", src)) == 1 and len(re.findall(r"u32 fmix32\(", src)) == 1, REGEN
    assert sh.N_TERM == (1 << 32) + 1


# ---- displaced pairs (test_gpu_hash_collisions.py::test_displaced_pairs_of_colliding_keys) ------------------------------------------------------
@pytest.mark.parametrize("n,founder", [(4, "a"), (4, "b"), (5, "a"), (5, "b"), (6, "ab"), (10, "ab"), (17, "ab")])
def test_displacing_pads_keep_the_collision_and_share_the_differing_loci_places(n, founder):
    H = FX["families"]["F2"]["n_haps"]
    for c in FX["families"]["F2"]["collisions"]:
        for where in WHERE:
            ka, kb = sh.displace(c, n, founder, where, FX)
            assert len(ka[0]) == len(kb[0]) == n and sh.set_hash(*ka) == sh.set_hash(*kb)
            for loci, masks in (ka, kb):
                assert np.all(np.diff(loci) > 0) and loci.min() >= 0 and loci.max() < FX["n_loci"] and masks.min() >= 1 and masks.max() < (1 << H)
            for s, own, other in (("a", ka, kb), ("b", kb, ka)):
                diff = set(own[0].tolist()) - set(other[0].tolist())
                assert len(diff) == 2
                if s in founder:                                       # every differing locus of a founder shares its place with a locus of the other key
                    assert all(any(sh.home_off(d) == sh.home_off(p) for p in other[0].tolist()) for d in diff)


def test_home_off_known_values():
    """g = 3: fmul = 2^16 + 2^13 + 2^10 + 2^7 + 2^4 + 2; consecutive loci step by one place, and loci seven apart share theirs (the
    paralog shape of test_gpu_parity.py)."""
    assert sum((1 << 16) >> (3 * i) for i in range(6)) == 74898
    assert [sh.home_off(x) for x in range(30001, 30009)] == [7, 1, 2, 3, 4, 5, 6, 7]
    assert len({sh.home_off(1 + 7 * k) for k in range(10)}) == 1


PINNED_GEOMETRY = [
    (r"for \(int i = 0; i < 6; \+\+i\) \{ f \+= x; x >>= g; \}", "pack_lgf: the factor is the sum of 2^16 >> (i * g), six terms"),
    (r"const u32 g = \(u32\)\(KS_SHORT \? 10 : 9\) - lg;", "pack_lgf: g = 9 - lg (10 - lg for ks_short)"),
    (r"return __builtin_amdgcn_ubfe\(__umul24\(key, H\.fmul\), 16u, H\.g\);", "home_off: bits [16, 16 + g) of the 24-bit product"),
    (r"u32 lgf = pack_lgf\(LGMAX\);", "a slice starts with the layout for the most reads"),
    (r"const u32 e4 = min\(est \* \(u32\)ECB_EST_MUL, 1u << LGMAX\);", "the next pass is laid out for ECB_EST_MUL tiles like the last"),
    (r"#define ECB_EST_MUL 4\b", "ECB_EST_MUL"),
    (r"#define ECB_LGMAX 6\b", "ECB_LGMAX"),
    (r"constexpr int LGMAX = KS_SHORT \? 7 : ECB_LGMAX;", "LGMAX"),
    (r"const u32 key = tag \| \(pr\.x \+ 1u\);", "the LDS key of a locus is locus + 1 under the read's tag"),
]


@pytest.mark.parametrize("pattern,what", PINNED_GEOMETRY, ids=[p[1] for p in PINNED_GEOMETRY])
def test_lds_place_of_a_locus_is_as_set_hash_restates_it(pattern, what):
    with open(os.path.join(CSRC, "k_stream.inc")) as f:
        n = len(re.findall(pattern, f.read()))
    assert n >= 1, "%s: the line changed -- restate tests/set_hash.py: home_off and rebuild test_gpu_hash_collisions.py::test_displaced_pairs_of_colliding_keys" % what
