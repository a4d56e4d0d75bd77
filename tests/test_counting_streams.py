"""``counting_streams`` -- the expected result of every test in ``test_gpu_counting.py`` -- against the C oracle (pinned to the
reference's goldens by ``test_c_oracle.py``), on every named stream small enough for both; and the arithmetic those tests rely on to
know which path of the counting pass an input takes (``ensure_counts``, ``k_build_work``, ``part_per`` in ``ecb.hip``), asserted
on the very inputs they use: a retune that moves a case off its edge fails here."""
import numpy as np
import pytest

from oracle import c_oracle

import counting_streams as cs


@pytest.mark.parametrize("name", sorted(cs.STREAMS))
def test_numpy_expectation_equals_the_c_oracle(name):
    st = cs.STREAMS[name]()
    exp = st.expected()
    assert int(exp["count"].sum()) == st.n_reads and np.array_equal(exp["first"], np.sort(exp["first"]))
    assert np.array_equal(np.bincount(exp["read_ec"], minlength=len(exp["count"])), exp["count"])
    if st.n_reads > cs.ORACLE_MAX_READS:
        return
    rid, loc, hf = st.tuples()
    o = c_oracle.ec_from_tuples(rid, loc, hf, cs.H, threads=3)
    for k in ("indptr", "indices", "data", "count"):
        assert np.array_equal(exp[k], o[k]), k
    s = exp["sizes"]
    assert (s["n_ecs"], s["nnz_a"], s["all_alignments"], s["valid_alignments"], s["n_reads"]) == \
        (len(o["count"]), len(o["indices"]), o["n_all"], o["n_valid"], o["n_reads"])


def test_big_ranking_stream_crosses_the_second_stretch_of_the_scan():
    st = cs.big_ranking_stream()
    assert st.n_reads == cs.BIG_READS and cs.SCB < cs.bitmap_lines(st.n_reads) <= 2 * cs.SCB
    assert 8388608 // cs.BM_LINE_READS == cs.SCB                  # read 8 388 608 opens line 16 384: the second stretch
    first = st.expected()["first"]
    assert {8388607, 8388608, st.n_reads - 1} <= set(first.tolist())
    assert (first < 8388607).sum() > 3000 and (first > 8388608).sum() > 1000


def test_ranges_per_table_size_and_knob():
    """Group 1: what (slots per range 2^bb, ranges nb) the table sizes and ECB_BIN_BITS values of
    test_slots_per_range_and_table_size give.  Tables are powers of two, so nb is one too: 2048 stands for 1025 .. 2048 ranges."""
    want = {(1 << 10, None): (11, 1), (1 << 10, 15): (15, 1), (1 << 16, None): (11, 32), (1 << 16, 15): (15, 2),
            (1 << 22, None): (13, 512), (1 << 22, 11): (11, 2048), (1 << 22, 12): (12, 1024), (1 << 22, 14): (14, 256),
            (1 << 22, 15): (15, 128), (1 << 24, 11): (11, 8192), (1 << 24, 12): (12, 4096), (1 << 27, None): (14, 8192),
            (1 << 27, 11): (14, 8192), (1 << 27, 15): (15, 4096), (1 << 28, None): (15, 8192), (1 << 28, 11): (15, 8192)}
    for (cap, knob), shape in want.items():
        assert cs.ranges(cap, knob) == shape, (cap, knob)
    nbs = {cs.ranges(cap, knob)[1] for cap in (1 << 10, 1 << 16, 1 << 22, 1 << 24, 1 << 27, 1 << 28) for knob in (None, 11, 12, 13, 14, 15)}
    assert {1, 1024, 2048, cs.STAGE_MAX_BUCKETS, 2 * cs.STAGE_MAX_BUCKETS} <= nbs          # one range; bpt 1, 2, 4; the plain scatter
    assert cs.ranges(1 << 29)[1] > cs.MAX_BUCKETS                                          # (refused by the library)
    assert cs.table_slots(1 << 10) == 1024 and cs.table_slots(1000) == 1024 and cs.table_slots((1 << 16) + 1) == 1 << 17


def test_partition_shapes_of_the_edge_read_counts():
    """Group 2.  G = min(512, ceil(R / 4096)) workgroups of part_per = ceil(R / G) rounded up to 4 reads.  What that gives at
    the read counts test_read_counts_on_the_partition_edges uses -- and what it can NOT give: the round-up wastes fewer than 4 G <= 2048
    reads in all while a workgroup's share is more than 2048 reads as soon as there are two, so no workgroup is ever empty and none
    but that of a one-read stream holds a single read (R = 1 is that case); the shortest last stretch of all is 2045 reads (R = 4097)."""
    shape = {r: cs.partition(r) for r in cs.EDGE_READS}
    for r in (1, 2, 3, 4, 5, 4095, 4096):
        assert shape[r][0] == 1 and shape[r][2] == [r]                 # one workgroup; R % 4 reads in its one-by-one tail
    assert shape[1][2] == [1]                                          # the one stream whose last workgroup holds a single read
    assert shape[4097] == (2, 2052, [2052, 2045])
    assert shape[8191] == (2, 4096, [4096, 4095]) and shape[8192] == (2, 4096, [4096, 4096])   # one stage of STAGE reads each
    assert cs.STAGE == 8192 and shape[8193] == (3, 2732, [2732, 2732, 2729])
    g, per, n = shape[2097151]
    assert (g, per) == (cs.PART_G, 4096) and n[:-1] == [4096] * 511 and n[-1] == 4095
    assert shape[2097152] == (cs.PART_G, 4096, [4096] * 512)
    g, per, n = shape[2097153]
    assert (g, per) == (cs.PART_G, 4100) and n[:-1] == [4100] * 511 and n[-1] == 2053        # short, not empty
    for r in list(range(2, 20000)) + list(range(2090000, 2100000, 7)) + [10 ** 7 + 1, 10 ** 8 + 3]:
        g, per, n = cs.partition(r)
        assert sum(n) == r and (g == 1 or min(n) >= 2045), r


CUT_CASES = {                      # stream -> (reads of its hottest template, work items of that template's range at 512 ranges if it is alone in it)
    "g3_one_ec_49152": (49152, 1), "g3_one_ec_49153": (49153, 2), "g3_one_ec_many_pieces": (1000001, 31),
    "g3_two_ecs_on_the_limit": (49153, 2), "g3_five_ecs": (300000, 10), "g3_hot_bunched_in_uniform": (120000, 4),
    "g3_hot_interleaved_in_uniform": (150001, 5)}


@pytest.mark.parametrize("name", sorted(CUT_CASES))
def test_cut_range_streams_are_cut(name):
    """Group 3: at both table sizes test_cut_ranges_through_every_sink uses (32 and 512 ranges) the hottest template alone holds
    more than 1.5 pieces -- its range is cut whatever slot it hashes to (``g3_one_ec_49152``: exactly 1.5 pieces of 32 768, the
    longest range that stays whole)."""
    st = cs.STREAMS[name]()
    hot, n_pieces = CUT_CASES[name]
    assert int(np.bincount(st.tpl).max()) == hot
    for cap in (1 << 16, 1 << 22):
        pc = cs.piece(st.n_reads, cs.ranges(cap)[1])
        if cap == 1 << 22:
            assert pc == cs.PIECE_MIN and cs.pieces(hot, pc) == n_pieces
        if name == "g3_one_ec_49152":
            assert pc == cs.PIECE_MIN and hot == pc + pc // 2 and cs.pieces(hot, pc) == 1
        else:
            assert hot > pc + pc // 2 and cs.pieces(hot, pc) >= 2
        assert 2 * len(np.unique(st.tpl)) <= cap and len(np.unique(st.tpl)) < 256          # the table never grows (see the GPU test)
