"""``contract_streams`` -- the inputs of ``test_gpu_tuple_contract.py`` -- checked on the CPU: every base and near-miss stream obeys the tuple
contract and the C oracle takes it; every break breaks exactly the rules it is named after, in the words it names and no others; the
cancelling breaks are exactly those that the stream kernel's check (per lane: sum of the steps against the number of odd ones) lets
through -- the open hole, which the GPU tests leave out; and an index out of range in a record that does not pass the filter changes nothing."""
import numpy as np
import pytest

from oracle import c_oracle

import contract_streams as cs
import refusal_streams as rs
from tuple_contract import obeys_contract

KINDS = sorted(cs.KINDS)


def _oracle(t, kind):
    return c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], kind.n_haps, threads=2)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a) and sorted(a) == sorted(b)


def test_geometry():
    assert rs._source("ecb.hip").count(cs.PLAN_RULE) == 1, "plan_stream changed: restate it in contract_streams.slice_edges"
    assert cs.slice_edges(cs.N) == [0, 2 * cs.WT, 4 * cs.WT] and cs.N - 4 * cs.WT == 100          # two slices of two tiles, and the short tile
    xs = sorted(cs.PLACES.values())
    assert len(set(xs)) == len(xs) == 28 and {x % 4 for x in xs} == {0, 1, 2, 3}
    assert {cs.WT, cs.WT + 255, cs.WT + 256, 2 * cs.WT - 1, 2 * cs.WT}.issubset(xs) and any(x > 4 * cs.WT for x in xs)
    assert cs.in_one_lane(cs.WT, 1) and cs.in_one_lane(cs.WT + 2, 1) and not cs.in_one_lane(cs.WT + 3, 1) and not cs.in_one_lane(cs.WT + 2, 2)


@pytest.mark.parametrize("name", KINDS)
def test_base_and_near_miss_streams_obey_the_contract(name):
    kind = cs.KINDS[name]
    for which, t in [(None, kind.base)] + list(enumerate(kind.near_miss)):
        assert len(t["read_id"]) == cs.N and obeys_contract(t, kind.n_loci, kind.n_haps), which
        assert cs.broken_rules(t, kind.n_loci, kind.n_haps) == set()
        assert (t["read_id"][:cs.PREFIX] == 0xFFFFFFFF).all() and not cs.valid(t)[:cs.PREFIX].any() and t["read_id"][cs.PREFIX] == 0
        D, H, f = cs.old_phase_a(t)
        assert (D == H).all() and not f
        o = _oracle(t, kind)
        heads = cs.heads_of(t)
        assert o["n_reads"] == t["n_reads"] == len(heads) == int(t["read_id"][-1]) + 1 and o["n_all"] == cs.N and o["n_valid"] == int(cs.valid(t).sum())
        places = kind.places()
        if which is None:                              # the base stream: every place inside a read that goes on behind it
            assert all(not ((heads >= x - 2) & (heads <= x + 5)).any() for x in places.values())
        else:                                          # near miss j: a head on every place + j, alone in its lane group; in number 0 a read ends on every edge
            for p, x in places.items():
                assert (x in heads) == p.endswith("+%d" % which), (p, which)
            assert all((e in heads) == (which == 0) for e in cs.EDGES)
    t, lens = kind.base, np.diff(np.r_[cs.heads_of(kind.base), cs.N])
    if name in ("mid", "giant"):
        small = lens[lens <= cs.WT]
        assert 12 <= cs.WT / small.mean() <= 20 and (name == "giant" or abs(cs.valid(t)[cs.PREFIX:].mean() - 0.5) < 0.01)
    if name == "long":                                 # passes laid out for few reads: a handful of reads per tile, each within what a read may carry over
        assert lens.min() >= 150 and np.median(lens) <= 250 and kind.distinct <= rs.CMAX
    if name == "short":                                # pick_variant: fewer than seven records per read, at most eight haplotypes
        assert cs.N < 7 * t["n_reads"] and kind.n_haps <= 8 and kind.hinted and np.median(lens) <= 6
    if name == "giant":                                # more loci than the table of a pass has room for entries: deferred to k_slow, whatever the tiling
        g = lens.max()
        assert g > cs.WT and len(set(t["locus"][kind.giant[0]:kind.giant[1]][cs.valid(t)[kind.giant[0]:kind.giant[1]]].tolist())) > cs.WT + rs.CMAX
        assert all(kind.giant[0] < x < kind.giant[1] - 8 for p, x in places.items() if p.startswith("giant"))
    else:
        assert lens.max() <= cs.WT


@pytest.mark.parametrize("name", KINDS)
def test_every_run_counter_break_breaks_its_rule_and_nothing_else(name):
    kind = cs.KINDS[name]
    cases = cs.run_counter_cases(kind)
    assert len(cases) == len(kind.places()) * len(cs.RUN_COUNTER)
    assert {l for l, _, _, _ in cs.run_counter_cases(kind, every=False)} < {l for l, _, _, _ in cases}
    n_cancel = 0
    for label, b, which, x in cases:
        t = kind.stream(which)
        heads = set(cs.heads_of(t).tolist())
        assert (x in heads) == (b.needs == "head") and not any(i in heads for i in range(x + 1, x + 3)), label
        u, words = b(t, x)
        assert cs.differing_words(t, u) <= words and ("read_id", x + b.at) in cs.differing_words(t, u), label
        assert cs.broken_rules(u, kind.n_loci, kind.n_haps) == set(b.rules) and not obeys_contract(u, kind.n_loci, kind.n_haps), label
        if b.width is not None:                         # back on course: the rest of the stream is the base's, its last read id too
            assert len(words) == b.width and u["read_id"][-1] == t["read_id"][-1], label
        D, H, f = cs.old_phase_a(u)
        # the two quantities the earlier check compared are equal, and no odd step sits on a filtered record: it let the stream through
        assert ((D == H).all() and not f) == b.cancels(x), label
        n_cancel += b.cancels(x)
    assert n_cancel >= 2 * len(kind.places())
    today = cs.run_counter_cases(kind, refused_today=True)             # what the GPU tests run: none of the open hole, everything else
    assert len(today) == len(cases) - n_cancel and all(not b.cancels(x) for _, b, _, x in today)


@pytest.mark.parametrize("name", KINDS)
def test_index_breaks(name):
    kind = cs.KINDS[name]
    t = kind.base
    base = _oracle(t, kind)
    v = cs.valid(t)
    for place in ("lane17+0", "short tile+1") + (("giant+0",) if kind.giant else ()):
        xp, xf = cs.record_near(t, kind.places()[place], True), cs.a_filtered_record(t, kind.places()[place])
        assert v[xp] and not v[xf]
        for label, fn, rule, _, _ in cs.index_breaks(kind):
            u, words = fn(t, xp)
            assert cs.differing_words(t, u) == words and len(words) == 1 and cs.broken_rules(u, kind.n_loci, kind.n_haps) == {rule}, label
            u, words = fn(t, xf)                       # in a record that does not pass: no rule broken, and the result is the base stream's
            assert cs.differing_words(t, u) == words and len(words) == 1 and cs.broken_rules(u, kind.n_loci, kind.n_haps) == set(), label
            assert _same(_oracle(u, kind), base), label
        for bit in (14, 15):                           # ignored bits (ecb.h), in a record that passes: the base stream's result
            u, words = cs.set_bit(t, xp, bit)
            assert words == {("hapflag", xp)} and cs.broken_rules(u, kind.n_loci, kind.n_haps) == set() and _same(_oracle(u, kind), base), bit
