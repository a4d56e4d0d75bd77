"""``racing_streams.py`` judged without a GPU: the lines of ``plan_stream`` it restates are pinned (a retune fails here and names the helper to
rebuild), its streams sit on the slices of the launch, and every family has the shape its test on the GPU relies on."""
import os
import re

import numpy as np
import pytest

import racing_streams as rs
import set_hash as sh

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")

# the lines of ecb.hip that racing_streams.plan_slices restates, in their order
PLAN_LINES = [
    r"h->resident_blocks\[i\] = \(u64\)std::max\(cus, 1\) \* std::max\(bpc, 1\);",
    r"h->rounds = getenv\(\"ECB_ROUNDS\"\) \? std::max\(1, atoi\(getenv\(\"ECB_ROUNDS\"\)\)\) : 24;",
    r"h->min_tiles = getenv\(\"ECB_MIN_TILES\"\) \? std::max\(2, atoi\(getenv\(\"ECB_MIN_TILES\"\)\)\) : 32;",
    r"const u64 res_waves = resident_blocks \* NWAVE;",
    r"u64 waves = std::min<u64>\(res_waves \* rounds, std::max<u64>\(n / \(MIN_TILES \* WT\), res_waves\)\);",
    r"waves = std::min<u64>\(waves, \(n \+ 2 \* WT - 1\) / \(2 \* WT\)\);",
    r"waves = std::max<u64>\(waves, 1\);",
    r"u64 chunk = \(n \+ waves - 1\) / waves;",
    r"chunk = \(chunk \+ WT - 1\) / WT \* WT;",
    r"waves = \(n \+ chunk - 1\) / chunk;",
    r"P->slices = waves; P->chunk = chunk;",
    r"P->blocks = std::min<u64>\(\(waves \+ NWAVE - 1\) / NWAVE, resident_blocks\);",
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_lines_of_plan_stream_the_helper_restates():
    src = _source("ecb.hip")
    at = 0
    for pat in PLAN_LINES:
        found = [m.start() for m in re.finditer(pat, src)]
        assert len(found) == 1, "plan_stream changed (%s): rebuild racing_streams.plan_slices and aligned_slices around it" % pat
        assert found[0] > at, "plan_stream's lines changed their order: rebuild racing_streams.plan_slices"
        at = found[0]
    assert re.search(r"constexpr int TPB = 256;", src) and re.search(r"constexpr int NWAVE = TPB / 64;", src)     # four waves per workgroup
    assert rs.WT == 512 and "static_assert(WT == 512" in _source("k_stream.inc")
    cmax = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*CMAX\s*=\s*([^;,]+)[;,]", _source("k_stream.inc"))
    assert [c.strip() for c in cmax] == ["KS_SHORT ? 64 : 80"] and rs.CMAX_STD == 80


@pytest.mark.parametrize("res_waves", [1024, 4096, 5120, 16384])
@pytest.mark.parametrize("rounds,min_tiles", [(24, 32), (1, 2), (1, 1000), (64, 2)])
def test_a_batch_of_whole_slices_is_cut_into_them_whatever_the_knobs(res_waves, rounds, min_tiles):
    for S in (1, 2, 63, 64, 96, 255, 256):
        assert rs.plan_slices(S * rs.SLICE, res_waves, rounds, min_tiles) == (S, rs.SLICE) and rs.aligned_slices(S * rs.SLICE) == S
    assert rs.plan_slices(64 * rs.SLICE + 512, res_waves, rounds, min_tiles) != (64, rs.SLICE)      # (off the grid the restatement says nothing)
    with pytest.raises(AssertionError):
        rs.aligned_slices(257 * rs.SLICE)
    with pytest.raises(AssertionError):
        rs.aligned_slices(64 * rs.SLICE + 512)


def test_the_builder_pads_with_repeats_and_refuses_what_cannot_be_aligned():
    rng = np.random.default_rng(1)
    reads = [rs.read_of(k) for k in rs.short_keys(rng, 40)]
    t = rs.build([reads, reads[::-1], reads[:7]])
    assert len(t["read_id"]) == 3 * rs.SLICE and t["n_slices"] == 3
    for s, part in enumerate((reads, reads[::-1], reads[:7])):
        keys = rs.slice_keys(t, s)
        own = [rs.key_of(r[0], 1 << r[1]) for r in part]
        assert keys[:len(own)] == own and set(keys) == set(own) and len(keys) == t["slice_reads"][s] > len(own)
    with pytest.raises(AssertionError):
        rs.build([reads * 30])                                   # more than a slice holds
    with pytest.raises(AssertionError):
        rs.build([[rs.covering(reads[0], 1000)]])                # nothing short enough to pad with
    bad = dict(t, read_id=np.concatenate([t["read_id"][:1], t["read_id"][:-1]]))
    with pytest.raises(AssertionError):
        rs.assert_aligned(bad)                                   # a slice that starts inside a read


@pytest.mark.parametrize("name", sorted(rs.FAMILIES))
def test_every_family_sits_on_the_slices_and_the_oracle_counts_its_ecs(name):
    t, info, exp = rs.family(name)
    rs.assert_aligned(t)
    n = len(t["read_id"])
    assert n <= 262144 and n // rs.SLICE == {"same_order_256": 256, "growth": 96}.get(name, 64)
    assert len(exp["count"]) == info["n_ecs"] and exp["n_reads"] == t["n_reads"] and exp["n_valid"] == exp["n_all"] == n
    assert "pos" in t if name == "ranges" else "pos" not in t


def _firsts(t, s, k):
    return rs.slice_keys(t, s)[:k]


def test_same_order_and_rotated_slices():
    t, info = rs.family("same_order", oracle=False)
    assert all(_firsts(t, s, 300) == info["keys"] for s in (0, 1, 31, 63))
    assert all(1 <= len(k[0]) <= 3 for k in info["keys"]) and len(set(info["keys"])) == 300
    t, info = rs.family("rotated", oracle=False)
    for s in (0, 1, 2, 5, 63):
        k = s * rs.PASS % 300
        assert _firsts(t, s, 300) == info["keys"][k:] + info["keys"][:k]
    assert _firsts(t, 1, 64) == _firsts(t, 0, 128)[64:]           # slice 1 founds in its first pass what slice 0 founds in its second


def test_same_slot_pairs_share_a_slot_and_not_a_hash():
    t, info = rs.family("same_slot", oracle=False)
    slots = set()
    for a, c in info["pairs"]:
        ha, hc = rs.hash_of(a), rs.hash_of(c)
        assert a != c and ha != hc and (ha ^ hc) & (rs.CAP_SMALL - 1) == 0
        slots.add(ha & (rs.CAP_SMALL - 1))
    assert len(slots) == len(info["pairs"]) == 150
    flat = [k for p in info["pairs"] for k in p]
    assert _firsts(t, 0, 300) == _firsts(t, 62, 300) == flat
    assert _firsts(t, 1, 300) == _firsts(t, 63, 300) == [k for a, c in info["pairs"] for k in (c, a)]


def test_same_hash_pairs_collide_under_the_restated_hash_in_the_same_place():
    t, info = rs.family("same_hash", oracle=False)
    assert len(info["colliding"]) == 24
    assert sorted({len(a[0]) for a, _ in info["colliding"]}) == list(rs.COLLISION_LENGTHS)
    assert sorted({len(b[0]) - len(a[0]) for a, b in info["colliding"]}) == [0, 1]          # F2 | N23
    even, odd = rs.slice_keys(t, 0), rs.slice_keys(t, 1)
    assert even == rs.slice_keys(t, 62) and odd == rs.slice_keys(t, 63)
    for i, (a, b) in enumerate(info["colliding"]):
        assert a != b and rs.hash_of(a) == rs.hash_of(b)
        assert even[3 * i] == a and odd[3 * i] == b                 # the same pass position, the other key
    other = lambda keys: [k for i, k in enumerate(keys[:124]) if i % 3 or i >= 72]          # (behind the 124 reads of a slice: its padding)
    assert other(even) == other(odd) and len(other(even)) == 100


def test_long_keys_giants_growth_and_ranges():
    t, info = rs.family("long_keys", oracle=False)
    assert sorted({len(k[0]) for k in info["longs"]}) == [6, 16, 17, 40]
    assert all(set(info["longs"]) <= set(rs.slice_keys(t, s)) for s in (0, 63))
    for name in ("giants_loci81", "giants_colliding"):
        t, info = rs.family(name, oracle=False)
        assert info["n_long"] == 64 and all(len(g[0]) in (81, 81 + (name == "giants_colliding")) for g in info["giants"])
        rid = t["read_id"]
        for s in (0, 1, 63):                                        # the slice's first read covers its first tile, on 81 loci and more than CMAX entries
            a = s * rs.SLICE
            assert (rid[a:a + rs.WT] == rid[a]).all() and rid[a + rs.WT] == rid[a] + 1
            assert rs.slice_keys(t, s)[0] == info["giants"][s % len(info["giants"])]
        if name == "giants_colliding":
            assert rs.hash_of(info["giants"][0]) == rs.hash_of(info["giants"][1]) and info["giants"][0] != info["giants"][1]
    t, info = rs.family("growth", oracle=False)
    assert info["n_ecs"] == 3000 > rs.CAP_SMALL
    for s in (0, 5, 6, 95):
        assert _firsts(t, s, 500) == info["keys"][s % 6 * 500:(s % 6 + 1) * 500]
    t, info = rs.family("ranges", oracle=False)
    t0, _ = rs.family("same_order", oracle=False)
    assert all(np.array_equal(t[k], t0[k]) for k in ("read_id", "locus", "hapflag"))
    mn, mx = rs.range_minmax(t)
    cell = np.unique(t["locus"].astype(np.int64) * rs.H + (t["hapflag"] >> 16))
    assert (mn[cell] < mx[cell]).all() and (mn[cell] >= 1000).all() and (mn != np.iinfo(np.int32).max).sum() == len(cell)
    first = t["pos"].reshape(64, rs.SLICE)                          # the extremes come from different slices, not from slice 0 alone
    assert (first.argmin(0) != 0).any() and (first.argmax(0) != 0).any() and len(set(first.argmin(0).tolist())) > 8


def test_the_merge_shards():
    t, info = rs.merge_shard()
    from oracle import c_oracle
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], rs.H, threads=4)
    assert len(exp["count"]) == info["n_ecs"] == t["n_reads"]
    assert len(info["colliding"]) == 24 and all(rs.hash_of(a) == rs.hash_of(b) and a != b for a, b in info["colliding"])
    w = rs.concatenated(t)
    assert w["n_reads"] == 8 * t["n_reads"] and len(w["read_id"]) == 8 * len(t["read_id"]) and (np.diff(w["read_id"].astype(np.int64)) >= 0).all()
    assert sh.set_hash(np.array([5]), np.array([1])) == rs.hash_of(((5,), (1,)))
