"""The read-counting pass behind ``k_stream`` -- ``ensure_counts`` and the ranking in ``ecb_finalize``: ``k_part_hist`` ->
``k_scan_lb`` -> ``k_part_scatter_staged`` | ``k_part_scatter`` -> ``k_build_work`` -> ``k_count_bins`` -> ``k_popc`` ->
``k_scan_lb`` -> ``k_rank`` -- on every path it picks at run time, EC by EC.

A wrong count here does not crash and mostly keeps ``sum(N) == n_reads``, so everything is compared bit for bit: ``dataN``, CSR ``A``,
the EC id of every read and the sizes ``finalize`` returns, against ``counting_streams`` (numpy on the stream's make-up) and, up to
about a million reads, against the C oracle through ``test_gpu_parity._check``.  ``test_counting_streams.py`` (CPU) holds the numpy
expectation against the C oracle and asserts, on these very inputs, the arithmetic that says which path each one takes;
``test_threshold_constants.py`` pins the constants of ``ecb.hip`` behind that arithmetic.

The table never grows in the cases that rely on its size.  ``ecb.hip`` grows it (x 4) only (a) before a batch while
``n_ecs * 2 > cap`` and (b) when a read finds no place within MAX_PROBE = 256 probes; the handle does not report its capacity.  The
cases of groups 2 - 4 and 6 hold fewer than 256 ECs in tables of at least 1024 slots, which rules out both; group 1 keeps the table
less than one seventh full."""
import numpy as np
import pytest

from alntools_amd import ecb
from oracle import c_oracle

import counting_streams as cs
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

KNOB = "ECB_BIN_BITS"
_cache = {}


def _get(name):
    """-> (stream, its tuples, what it must give, the C oracle's result or None), made once."""
    if name not in _cache:
        st = cs.STREAMS[name]()
        t = st.tuples()
        orc = c_oracle.ec_from_tuples(t[0], t[1], t[2], cs.H, threads=8) if st.n_reads <= cs.ORACLE_MAX_READS else None
        _cache[name] = (st, t, st.expected(), orc)
    return _cache[name]


def _push(b, t, device):
    if device:
        import torch
        d = [torch.from_numpy(a.view(np.int32)).cuda() for a in t]
        torch.cuda.synchronize()
        b.push_device(*d)
        return d                                                          # (alive until the caller is done with the handle)
    b.push(*t)


def _same(out, sizes, exp, what):
    assert sizes == exp["sizes"], what
    for a, k in (("indptrA", "indptr"), ("indicesA", "indices"), ("dataA", "data"), ("dataN", "count")):
        assert np.array_equal(out[a], exp[k]), (what, a)
    assert out["indptrN"].tolist() == [0, len(exp["count"])] and np.array_equal(out["indicesN"], np.arange(len(exp["count"]))), what
    if "read_ec" in out:
        assert np.array_equal(out["read_ec"], exp["read_ec"]), (what, "read_ec")


def _finalize_and_compare(b, exp, orc, what, read_ec=True):
    sizes = b.finalize()
    out = b.export()
    if read_ec:
        out["read_ec"] = b.export_read_ec()
    _same(out, sizes, exp, what)
    if orc is not None:
        _check(out, sizes, orc)
    return out, sizes


def _run(b, name, device, what=None):
    st, t, exp, orc = _get(name)
    keep = _push(b, t, device)
    r = _finalize_and_compare(b, exp, orc, what or name)
    del keep
    return r


# ---- 1. slots per range x table size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,n_tpl", [(1 << 10, 200), (1 << 16, 1 << 13), (1 << 22, 1 << 19), (1 << 24, 1 << 19), (1 << 27, 1 << 19),
                                       (1 << 28, 1 << 19)])
def test_slots_per_range_and_table_size(cap, n_tpl, monkeypatch):
    """ECB_BIN_BITS unset and 11 .. 15 on tables of 2^10 (one range) .. 2^28 slots (2^15 slots per range forced; 16 GB: one such
    handle at a time), ONE handle per table size, reset between streams -- a work list, a list of occupied slots or an LDS attribute
    left over from the stream before shows.  Streams of a million reads: uniform, one hot template in every other read, three hot
    templates in runs of 3000; from 2^22 slots on also every EC once.  2^24 and 2^27 slots give 4096 and 8192 ranges (the staged
    and the plain scatter), 2^22 slots 1024 and 2048 (1, 2 ranges per thread of the staged scatter's scan; 4096: 4) --
    test_counting_streams.py::test_ranges_per_table_size_and_knob.  A knob value that gives a (bb, nb) this handle has already run
    repeats the bunched stream only."""
    names = ["g1_hot3_bunched_%d" % n_tpl, "g1_uniform_%d" % n_tpl, "g1_hot1_interleaved_%d" % n_tpl] + (["g1_each_once"] if cap >= 1 << 22 else [])
    most = max(_get(n)[2]["sizes"]["n_ecs"] for n in names)
    assert cs.table_slots(cap) == cap and (most < 256 or most * 7 <= cap)
    import torch
    dev = {n: [torch.from_numpy(a.view(np.int32)).cuda() for a in _get(n)[1]] for n in names}
    torch.cuda.synchronize()
    seen = set()
    with ecb.EcBuilder(max(_get(n)[0].n_loci for n in names), cs.H, ec_capacity=cap) as b:
        for knob in (None, 15, 11, 14, 12, 13):
            if knob is None:
                monkeypatch.delenv(KNOB, raising=False)
            else:
                monkeypatch.setenv(KNOB, str(knob))
            shape = cs.ranges(cap, knob)
            for name in (names if shape not in seen else names[:1]):
                st, t, exp, orc = _get(name)
                b.reset()
                b.push_device(*dev[name])
                _finalize_and_compare(b, exp, orc, (name, cap, knob, shape))
            seen.add(shape)
    monkeypatch.delenv(KNOB, raising=False)


# ---- 2. read counts on the partition's edges -----------------------------------------------------------------------------------------
def test_read_counts_on_the_partition_edges():
    """1 .. 5, 4095 .. 4097, 8191 .. 8193 and 2 097 151 .. 2 097 153 reads, uniform over 100 templates and degenerate (1, 2 or 5
    templates), on one handle of 2^16 slots (32 ranges), long and short streams in turn.  The shapes of the partition's
    workgroups at these read counts -- and why no read count leaves a workgroup empty or, beyond a one-read stream, with a single
    read -- are asserted in test_counting_streams.py::test_partition_shapes_of_the_edge_read_counts."""
    reads = sorted(cs.EDGE_READS)
    order = [r for pair in zip(reversed(reads), reads) for r in pair][:len(reads)]          # longest, shortest, second longest ...
    assert sorted(order) == reads
    with ecb.EcBuilder(3 * 100, cs.H, ec_capacity=1 << 16) as b:
        for r in order:
            for kind in ("uniform", "degenerate"):
                name = "g2_%s_%d" % (kind, r)
                b.reset()
                _run(b, name, device=r > 5000)
                if r > cs.ORACLE_MAX_READS:
                    _cache.pop(name)


# ---- 3. cut ranges, every sink -------------------------------------------------------------------------------------------------------
CUT = ["g3_one_ec_49152", "g3_one_ec_49153", "g3_one_ec_many_pieces", "g3_two_ecs_on_the_limit", "g3_five_ecs",
       "g3_hot_bunched_in_uniform", "g3_hot_interleaved_in_uniform"]


def _entries(eng, n):
    """A handle's exported table -> (first read, reads) of every entry, sorted by first read."""
    ent, _, eoff, _ = eng.table_export_parts(0, 3)
    assert eoff[0] == 0 and eoff[-1] == n
    w = ent[:n * 4].view(-1, 4)[:, 2].cpu().numpy()
    first, count = (~(w >> 32)) & 0xFFFFFFFF, w & 0xFFFFFFFF
    o = np.argsort(first)
    return first[o], count[o]


@pytest.mark.parametrize("cap", [1 << 16, 1 << 22])
@pytest.mark.parametrize("name", CUT)
def test_cut_ranges_through_every_sink(name, cap):
    """One template alone holds more than 1.5 pieces of the work list, so its range is cut into pieces that add with atomics and
    list their slots the second way, whatever slot it hashes to -- 2 pieces, many, and a range of exactly 1.5 pieces, which stays
    whole (test_counting_streams.py::test_cut_range_streams_are_cut asserts piece and the inequality for these streams at these
    table sizes; degenerate streams in a large table make a range's length exact).  Fewer than 256 ECs: the table stays at
    ``cap``.  Sinks: (a) finalize, (d) a second finalize, (b) a table export first -- the pass lists the slots for itself -- and
    finalize on the same handle, then (d) again."""
    import torch
    from alntools_amd import dist as ecdist
    st, t, exp, orc = _get(name)
    assert exp["sizes"]["n_ecs"] < 256 and cs.table_slots(cap) == cap
    with ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=cap) as b:
        keep = _push(b, t, device=True)
        first, s1 = _finalize_and_compare(b, exp, orc, (name, "finalize"))
        again, s2 = _finalize_and_compare(b, exp, orc, (name, "second finalize"))
        assert s1 == s2 and all(np.array_equal(first[k], again[k]) for k in first)
        b.reset()
        b.push_device(*keep)
        eng = ecdist.GpuEngine(b, torch.device("cuda:0"))
        f, c = _entries(eng, exp["sizes"]["n_ecs"])
        assert np.array_equal(f, exp["first"]) and np.array_equal(c, exp["count"]), (name, "table export")
        _finalize_and_compare(b, exp, orc, (name, "finalize after a table export"))
        _finalize_and_compare(b, exp, orc, (name, "second finalize after a table export"))


@pytest.mark.parametrize("name", ["g3_one_ec_many_pieces", "g3_five_ecs", "g3_hot_interleaved_in_uniform"])
def test_cut_ranges_in_two_shards_merged_by_key_range_and_adopted(name):
    """Sink (c): the stream in two shards, both holding the hot template in a cut range (asserted below); every shard's table exported
    in two key ranges, range q of both merged on a handle of its own, the two results adopted by a root handle: the counts are the
    sums, the order that of first appearance over the whole stream."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    st, t, exp, orc = _get(name)
    cap, cut = 1 << 22, int(st.n_reads * 0.45)
    shards = [st.shard(0, cut), st.shard(cut, st.n_reads)]
    exported, base, n_all = [], 0, 0
    for sh in shards:
        pc = cs.piece(sh.n_reads, cs.ranges(cap)[1])
        assert int(np.bincount(sh.tpl).max()) > pc + pc // 2 and len(np.unique(sh.tpl)) < 256
        b = ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=cap)
        keep = _push(b, sh.tuples(), device=True)
        exported.append(ecdist.GpuEngine(b, dev).table_export_parts(base, 2))
        assert b.counters()[2] == sh.n_reads
        n_all += b.counters()[0]
        base += sh.n_reads
        b.close()
        del keep
    root = ecdist.GpuEngine(ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=1 << 10), dev)
    for q in range(2):
        part = ecdist.GpuEngine(ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=1 << 12), dev)
        part.table_merge_many([(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                               for ent, prs, eoff, poff in exported if eoff[q + 1] > eoff[q]])
        pe_n, pp_n, _ = part.table_sizes()
        pe, pp = part.table_export(0)
        root.table_adopt(pe, pe_n, pp, pp_n)
        part.b.close()
    root.add_counters(n_all, n_all, base)
    _finalize_and_compare(root.b, exp, orc, (name, "adopted"), read_ec=False)       # (per-read EC ids are not kept across a merge)
    _finalize_and_compare(root.b, exp, orc, (name, "adopted, second finalize"), read_ec=False)
    root.b.close()


# ---- 4. hot value per wave -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1 << 10, 1 << 16])
def test_runs_of_one_slot_in_a_wave(cap):
    """Runs of one template of 1 .. 9, 63 .. 65 and 8 x 1024 +- 1 reads, each followed at once by a run of a second hot template,
    between uniform reads: k_count_bins adds a value once per wave when eight or more of its lanes hold it (a lane loads eight
    consecutive elements, so runs of 63 .. 65 put 7, 8 and 9 equal lanes into one of its steps), the others one by one.  One range
    (2^10 slots: the elements keep the stream's order but for the shuffling within a stage) and 32."""
    with ecb.EcBuilder(_get("g4_runs")[0].n_loci, cs.H, ec_capacity=cap) as b:
        _run(b, "g4_runs", device=False)
        b.reset()
        _run(b, "g4_runs", device=True)


# ---- 5. ranking ----------------------------------------------------------------------------------------------------------------------
def test_first_appearances_on_the_bitmap_line_ends():
    """ECs first seen at reads 510 .. 513, 16 383, 16 384 and the last read, every other read a repeat of an earlier EC: bit_rank
    on the ends of the bitmap's 512-read lines and 32-read words."""
    st, t, exp, orc = _get("g5_line_firsts")
    assert set(cs.LINE_FIRSTS + (st.n_reads - 1,)) <= set(exp["first"].tolist())
    with ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=1 << 10) as b:
        _run(b, "g5_line_firsts", device=False)


def test_ranking_across_the_first_stretch_of_the_scan():
    """8 388 608 + 4096 one-record reads pushed from device memory, ECs first seen at reads 8 388 607 and 8 388 608 and thousands
    more on both sides: the scan over the bitmap lines' popcounts runs over two stretches, joined by the decoupled look-back.
    numpy alone says what this gives (test_counting_streams.py::test_big_ranking_stream_crosses_the_second_stretch_of_the_scan)."""
    st = cs.big_ranking_stream()
    exp = st.expected()
    assert cs.bitmap_lines(st.n_reads) > cs.SCB
    with ecb.EcBuilder(st.n_loci, cs.H, ec_capacity=1 << 16) as b:
        keep = _push(b, st.tuples(), device=True)
        _finalize_and_compare(b, exp, None, "big ranking stream")
        del keep


# ---- 6. reads after a merge or an adopt ----------------------------------------------------------------------------------------------
def test_no_reads_after_a_merge_or_an_adopt_and_the_handle_stays_usable():
    """``include/ecb.h`` lets no read into a handle whose counts are made: a merge counts the handle's own reads first, an adopt
    wants an empty handle.  So push, merge, push again is refused (ECB_ERR_STATE), as are an adopt into a handle that holds reads
    and a push into one that adopted -- k_count_bins never sees an occupied slot without a read of the handle's own in a whole
    range -- and after each refusal the handle finalizes to what it held: own reads plus merged entries, counts added, in order of
    first appearance over both."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    own, t_own, _, _ = _get("g6_own")
    other, t_other, exp_other, orc_other = _get("g6_other")
    both = cs.concat(own, other)
    exp = both.expected()
    tb = both.tuples()
    orc = c_oracle.ec_from_tuples(tb[0], tb[1], tb[2], cs.H, threads=8)
    src = ecdist.GpuEngine(ecb.EcBuilder(own.n_loci, cs.H, ec_capacity=1 << 12), dev)
    keep = [_push(src.b, t_other, device=True)]
    ne, npairs, nreads = src.table_sizes()
    ent, prs = src.table_export(own.n_reads)                              # first reads counted on from the handle's own
    with ecb.EcBuilder(own.n_loci, cs.H, ec_capacity=1 << 12) as b:
        keep.append(_push(b, t_own, device=True))
        with pytest.raises(ecb.EcbError) as e:
            b.table_adopt_device(ent, ne, prs, npairs)
        assert e.value.code == -6
        b.table_merge_device(ent, ne, prs, npairs)
        with pytest.raises(ecb.EcbError) as e:
            b.push(*t_other)
        assert e.value.code == -6
        with pytest.raises(ecb.EcbError) as e:
            b.push_device(*keep[0])
        assert e.value.code == -6
        a, v, _ = src.counters()
        b.add_counters(a, v, nreads)
        _finalize_and_compare(b, exp, orc, "own reads + merged entries", read_ec=False)
    with ecb.EcBuilder(own.n_loci, cs.H, ec_capacity=1 << 10) as b:
        ent0, prs0 = src.table_export(0)
        b.table_adopt_device(ent0, ne, prs0, npairs)
        with pytest.raises(ecb.EcbError) as e:
            b.push(*t_own)
        assert e.value.code == -6
        a, v, _ = src.counters()
        b.add_counters(a, v, nreads)
        _finalize_and_compare(b, exp_other, orc_other, "adopted entries", read_ec=False)
    src.b.close()
