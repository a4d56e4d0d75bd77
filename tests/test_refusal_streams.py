"""``refusal_streams`` -- the inputs of ``test_gpu_refused_runs.py`` -- checked on the CPU: every stream obeys the tuple contract, the C
oracle accepts it, and it meets the margin that makes its outcome on the GPU independent of how the waves pack their arena chunks.  The
margins are conditions, computed from constants read out of the kernel sources: when one of those moves, this fails and names the stream
to resize."""
import re

import numpy as np
import pytest

from oracle import c_oracle

import refusal_streams as rs

STREAMS = [(c, w) for c in sorted(rs.CASES) for w in ("refused", "recovery")]


def test_the_arena_of_the_refused_handle_is_one_region_of_eight_chunks():
    assert len(re.findall(rs.ARENA_REGIONS_RULE, rs._source("ecb.hip"))) == 1, "arena_regions changed: restate it in refusal_streams.py"
    assert rs.arena_regions(rs.ARENA) == 1 and rs.ARENA == 8 * rs.ARENA_CHUNK
    assert rs.arena_regions(1 << 24) == rs.ARENA_REGIONS and rs.arena_regions(1 << 17) == 2      # (the control handle; two regions)
    assert rs.LONG > rs.INL and rs.LONG <= rs.CMAX_SHORT                                         # long keys, founded by the stream kernel itself


@pytest.mark.parametrize("case,which", STREAMS, ids=["%s-%s" % s for s in STREAMS])
def test_stream_obeys_the_contract_and_meets_its_margin(case, which):
    c = rs.CASES[case]
    t = getattr(c, which)
    assert rs.obeys_contract(t, c.n_loci, c.n_haps)
    o = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], c.n_haps, threads=2)
    keys = rs.read_keys(t)
    assert o["n_reads"] == t["n_reads"] == len(keys) and len(o["count"]) == len(set(keys)) and o["n_valid"] == o["n_all"] == len(t["read_id"])
    beyond = rs.key_pairs_beyond_the_slot(t)
    assert beyond == int(np.maximum(np.diff(o["indptr"]) - rs.INL, 0).sum())                     # (the oracle's rows say the same)
    if which == "refused":
        assert beyond >= 4 * rs.ARENA, "%s: the distinct keys need %d pairs of the arena, fewer than 4 x %d: add reads" % (case, beyond, rs.ARENA)
        assert len(t["read_id"]) < 100_000
    else:
        need = rs.recovery_need(t)
        assert beyond > 0 and 4 * need <= rs.ARENA, "%s: recovery may take %d pairs, more than %d / 4: take reads out" % (case, need, rs.ARENA)


def test_what_each_case_is_about():
    """The shape that sends each stream down its path: keys the stream kernel founds itself (no longer than a read may carry over a tile's
    end); six records per read for ks_short (``pick_variant``: fewer than seven); reads longer than a tile for k_slow, the recovery's too."""
    assert set(np.diff(np.flatnonzero(np.r_[1, np.diff(rs.STD.refused["read_id"]), 1]))) == {rs.LONG}
    t = rs.SHORT.refused
    assert len(t["read_id"]) == (rs.INL + 1) * t["n_reads"] < 7 * t["n_reads"] and t["n_reads"] >= 16_384 and rs.SHORT.n_haps <= 8
    assert rs.SHORT.n_loci < (1 << 25) - 2
    for t in (rs.SLOW.refused, rs.SLOW.recovery):
        assert np.bincount(t["read_id"]).max() > rs.WT
    assert np.bincount(rs.SLOW.refused["read_id"]).min() > rs.WT and rs.SLOW_LEN < 4096          # (within k_slow's LDS: SLOW_LDS)


def test_queue_stream():
    t, T, H = rs.queue_stream()
    assert rs.obeys_contract(t, T, H)
    keys = rs.read_keys(t)
    assert len(keys) == t["n_reads"] and all(len(k) == rs.CMAX + 1 for k in keys) and 200 <= t["n_reads"] <= 999
    # the last record of every whole tile is the last of a read's CMAX + 1 valid records, all in that tile
    ends = np.arange(rs.WT - 1, len(t["read_id"]), rs.WT)
    assert len(ends) >= 40
    for e in ends:
        assert (t["read_id"][e - rs.CMAX:e + 1] == t["read_id"][e]).all() and (t["hapflag"][e - rs.CMAX:e + 1] & 4 == 0).all()
        assert e + 1 == len(t["read_id"]) or t["hapflag"][e + 1] & 4 or t["read_id"][e + 1] == t["read_id"][e] + 1
    o = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H)
    assert o["n_reads"] == t["n_reads"] and o["n_valid"] == t["n_reads"] * (rs.CMAX + 1) < o["n_all"] == len(t["read_id"])
