"""GPU parity: libecb (through its C ABI) against the oracle on the same tuples.  Bit-exact."""
import json
import os

import numpy as np
import pytest

from alntools_amd import ecb, synth
from oracle import ec_oracle as orc

pytestmark = pytest.mark.gpu


def _expect(t, n_loci, n_haps, with_pos=False):
    return orc.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], n_loci, n_haps,
                              pos=t["pos"] if with_pos else None)


def _check(out, sizes, exp):
    assert sizes["n_ecs"] == len(exp["count"])
    assert sizes["all_alignments"] == exp["n_all"] and sizes["valid_alignments"] == exp["n_valid"]
    assert np.array_equal(out["indptrA"], exp["indptr"])
    assert np.array_equal(out["indicesA"], exp["indices"])
    assert np.array_equal(out["dataA"], exp["data"])
    assert np.array_equal(out["dataN"], exp["count"])
    assert out["indptrN"].tolist() == [0, len(exp["count"])]
    assert np.array_equal(out["indicesN"], np.arange(len(exp["count"])))


def _run_host(t, n_loci, n_haps, batch=None, ranges=False, **kw):
    with ecb.EcBuilder(n_loci, n_haps, track_ranges=ranges, **kw) as b:
        n = len(t["read_id"])
        step = batch or max(n, 1)
        for a in range(0, n, step):
            sl = slice(a, a + step)
            b.push(t["read_id"][sl], t["locus"][sl], t["hapflag"][sl], t["pos"][sl] if ranges else None)
        sizes = b.finalize()
        out = b.export()
        out["read_ec"] = b.export_read_ec()
        if ranges:
            out["ranges"] = b.export_ranges()
        return out, sizes


@pytest.fixture(scope="module")
def c1():
    spec = synth.SynthSpec(10000, 1000, 2)
    return spec, synth.generate(spec, 0, spec.n_reads)


def test_config1_matches_oracle_and_golden_bin(c1, golden_dir):
    spec, t = c1
    out, sizes = _run_host(t, spec.n_loci, spec.n_haps, ranges=True)
    exp = _expect(t, spec.n_loci, spec.n_haps, with_pos=True)
    _check(out, sizes, exp)
    assert np.array_equal(out["ranges"], exp["range"])
    w = orc.ecload_bytes(open(os.path.join(golden_dir, "g2_c1.bin"), "rb").read())
    for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN"):
        assert np.array_equal(out[k], w[k]), k
    g = json.load(open(os.path.join(golden_dir, "g2_c1.json")))
    assert sizes["valid_alignments"] == g["counters"]["# Valid Alignments"]
    assert sizes["n_reads"] == g["n_reads"]


@pytest.mark.parametrize("batch", [1, 7, 1000, 4097])
def test_reads_straddling_host_batches(c1, batch):
    spec, t = c1
    n = 3000 if batch == 1 else 40000
    tt = {k: (v[:n] if hasattr(v, "__len__") else v) for k, v in t.items()}
    out, sizes = _run_host(tt, spec.n_loci, spec.n_haps, batch=batch, max_batch_records=5000)
    _check(out, sizes, _expect(tt, spec.n_loci, spec.n_haps))


def test_read_ec_ids(c1):
    spec, t = c1
    out, sizes = _run_host(t, spec.n_loci, spec.n_haps)
    # the EC of read r, rebuilt from its own records, is row read_ec[r] of A
    exp = _expect(t, spec.n_loci, spec.n_haps)
    rows = {}
    for e in range(len(exp["count"])):
        sl = slice(exp["indptr"][e], exp["indptr"][e + 1])
        rows[tuple(zip(exp["indices"][sl].tolist(), exp["data"][sl].tolist()))] = e
    valid = orc.tuples_valid(t["hapflag"])
    rid = t["read_id"][valid].astype(np.int64)
    loc = t["locus"][valid].astype(np.int64)
    hap = (t["hapflag"][valid].astype(np.int64) >> 16) & 0xFF
    got = out["read_ec"]
    assert len(got) == sizes["n_reads"]
    cnt = np.bincount(got, minlength=sizes["n_ecs"])
    assert np.array_equal(cnt, exp["count"])
    for r in (0, 1, 17, 4242, sizes["n_reads"] - 1):
        m = rid == r
        d = {}
        for l, h in zip(loc[m].tolist(), hap[m].tolist()):
            d[l] = d.get(l, 0) | (1 << h)
        assert rows[tuple(sorted(d.items()))] == got[r]


def test_paired_end_8_haplotypes(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "g3_pe.json")))
    spec = synth.SynthSpec(**g["spec"])
    t = synth.generate(spec, 0, spec.n_reads)
    out, sizes = _run_host(t, spec.n_loci, spec.n_haps)
    _check(out, sizes, _expect(t, spec.n_loci, spec.n_haps))
    assert sizes["valid_alignments"] == g["counters"]["# Valid Alignments"]
    assert sizes["n_ecs"] == g["counters"]["# Equivalence Classes"]


def test_device_resident_push_and_table_growth():
    import torch
    spec = synth.SynthSpec(30000, 2000, 8)
    t = synth.generate(spec, 0, spec.n_reads)
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(t[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")}
    torch.cuda.synchronize()
    with ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1024) as b:   # forces deferrals + growth
        b.push_device(d["read_id"], d["locus"], d["hapflag"])
        sizes = b.finalize()
        out = b.export()
    _check(out, sizes, _expect(t, spec.n_loci, spec.n_haps))


def test_reads_bound_given_up_front_and_a_handle_reused_for_a_shorter_stream():
    """``ecb_hint_reads``: with the stream's read count bounded up front a device push does not ask the device for the batch's last
    read id; the result is the same, in one batch or several, with a table that has to grow, on a handle that held a LONGER
    stream before (its per-read slot ids are not cleared by ``reset``: every read of the new stream must overwrite its own),
    and a stream that runs past the bound is a contract error, not a write past the per-read array."""
    import torch
    dev = torch.device("cuda:0")
    big = synth.SynthSpec(50000, 3000, 8)
    small = synth.SynthSpec(21000, 700, 4, paired=True)
    tb, ts = synth.generate(big, 0, big.n_reads), synth.generate(small, 0, small.n_reads)
    db = {k: torch.from_numpy(tb[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")}
    exp_b = _expect(tb, big.n_loci, big.n_haps)
    n_reads_b = int(tb["read_id"][-1]) + 1
    with ecb.EcBuilder(big.n_loci, big.n_haps, ec_capacity=4096) as b:       # (grows while the hinted stream is pushed)
        b.hint_reads(n_reads_b)
        cuts = [0]
        for frac in (0.3, 0.55, 1.0):                                        # whole reads per batch
            c = int(len(tb["read_id"]) * frac)
            while c < len(tb["read_id"]) and tb["read_id"][c] == tb["read_id"][c - 1]:
                c += 1
            cuts.append(c)
        for a, e in zip(cuts[:-1], cuts[1:]):
            b.push_device(db["read_id"][a:e].clone(), db["locus"][a:e].clone(), db["hapflag"][a:e].clone())
        s = b.finalize()
        _check(b.export(), s, exp_b)
        # the same handle, a shorter stream of another shape (fewer loci: the builder is per (n_loci, n_haps), so a second one)
        b.reset()
        cut = cuts[1]
        b.hint_reads(int(tb["read_id"][cut - 1]) + 1)
        b.push_device(db["read_id"][:cut].clone(), db["locus"][:cut].clone(), db["hapflag"][:cut].clone())
        s = b.finalize()
        part = {k: tb[k][:cut] for k in ("read_id", "locus", "hapflag")}
        exp_p = orc.ec_from_tuples(part["read_id"], part["locus"], part["hapflag"], big.n_loci, big.n_haps)
        _check(b.export(), s, exp_p)
        got = b.export_read_ec()
        assert len(got) == int(tb["read_id"][cut - 1]) + 1
        # ... and without the bound again (the handle asks the device, as before)
        b.reset()
        b.hint_reads(0)
        b.push_device(db["read_id"], db["locus"], db["hapflag"])
        s = b.finalize()
        _check(b.export(), s, exp_b)
    ds = {k: torch.from_numpy(ts[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")}
    with ecb.EcBuilder(small.n_loci, small.n_haps) as b:
        b.hint_reads(int(ts["read_id"][-1]) + 1 - 5)                         # five reads too few
        with pytest.raises(ecb.EcbError) as e:
            b.push_device(ds["read_id"], ds["locus"], ds["hapflag"])
        assert e.value.code == -5                      # ECB_ERR_CONTRACT


def test_table_of_2_to_the_27_slots_counts_like_a_small_one():
    """Beyond 2^26 slots k_count's ranges hold 2^14 / 2^15 slots each (LDS counters as dynamic shared memory): same results."""
    import torch
    spec = synth.SynthSpec(30000, 2000, 8, paired=True)
    t = synth.generate(spec, 0, spec.n_reads)
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(t[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")}
    for cap in (1 << 27, 1 << 28):
        with ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=cap) as b:
            b.push_device(d["read_id"], d["locus"], d["hapflag"])
            sizes = b.finalize()
            out = b.export()
        _check(out, sizes, _expect(t, spec.n_loci, spec.n_haps))
    with pytest.raises(ecb.EcbError):
        with ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 29) as b:      # 32 GB of slots: allocates, counts refuse
            b.push_device(d["read_id"], d["locus"], d["hapflag"])
            b.finalize()


def _hand(records, n_haps):
    """records: list of (read_id, locus, hap, flag)"""
    a = np.array(records, dtype=np.int64).reshape(-1, 4)
    return dict(read_id=a[:, 0].astype(np.uint32), locus=a[:, 1].astype(np.uint32),
                hapflag=(a[:, 3] | (a[:, 2] << 16)).astype(np.uint32), pos=np.zeros(len(a), np.int32))


def test_reads_longer_than_a_tile():
    T, H = 5000, 4
    recs = [(0, 5, 1, 0), (0, 5, 2, 0)]
    big = [(1, (i * 7) % T, i % H, 0) for i in range(6000)] + [(1, 0, 0, 0)] * 3
    recs += big
    recs += [(2, 5, 2, 0), (2, 5, 1, 16)]                       # same EC as read 0
    recs += [(3, l, h, f) for (_, l, h, f) in reversed(big)]     # same EC as read 1, other order
    recs += [(3, 9, 0, 4)] * 5                                   # unmapped tail inside read 3
    recs += [(4, 4999, 3, 0)]
    t = _hand(recs, H)
    for batch in (None, 1500):
        out, sizes = _run_host(t, T, H, batch=batch)
        exp = _expect(t, T, H)
        _check(out, sizes, exp)
        assert exp["count"].tolist() == [2, 2, 1]


def test_filter_bits_and_leading_invalid_records():
    H = 2
    M = 0xFFFFFFFF
    recs = [(M, 0, 0, 4), (M, 0, 0, 4),                          # unmapped before any read
            (0, 1, 0, 0), (0, 1, 1, 0), (0, 2, 0, 0x4),          # unmapped inside read 0
            (0, 3, 0, 0x1 | 0x40), (0, 3, 1, 0x1 | 0x2 | 0x80),  # improper pair; read2
            (0, 3, 0, 0x1 | 0x2 | 0x40 | 0x1000), (0, 3, 0, 0x1 | 0x2 | 0x40 | 0x2000),
            (1, 3, 0, 0x1 | 0x2 | 0x40), (1, 3, 0, 0x1 | 0x2 | 0x40),   # duplicate collapses
            (2, 1, 1, 0), (2, 1, 0, 16), (2, 9, 1, 4)]
    t = _hand(recs, H)
    out, sizes = _run_host(t, 10, H)
    _check(out, sizes, _expect(t, 10, H))
    assert sizes["valid_alignments"] == 6 and sizes["n_reads"] == 3 and sizes["n_ecs"] == 2
    assert out["dataN"].tolist() == [2, 1] and out["dataA"].tolist() == [3, 1]


def test_errors_are_loud():
    with ecb.EcBuilder(4, 2) as b:
        b.push(np.array([0xFFFFFFFF], np.uint32), np.array([0], np.uint32), np.array([4], np.uint32))
        with pytest.raises(ecb.EcbError) as e:
            b.finalize()
        assert e.value.code == -7                      # ECB_ERR_EMPTY
    with ecb.EcBuilder(4, 2) as b:                     # run counter jumps by 2
        with pytest.raises(ecb.EcbError) as e:
            b.push(np.array([0, 2, 2], np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint32))
            b.finalize()
        assert e.value.code == -5
    with ecb.EcBuilder(4, 2) as b:                     # locus out of range
        with pytest.raises(ecb.EcbError) as e:
            b.push(np.array([0, 1], np.uint32), np.array([1, 4], np.uint32), np.zeros(2, np.uint32))
            b.finalize()
        assert e.value.code == -5
    with pytest.raises(ecb.EcbError):
        ecb.EcBuilder(4, 40)


@pytest.mark.parametrize("paired", [False, True])
def test_mid_size_device_vs_c_oracle_properties(paired):
    """200k reads: totals and order-independence checks that need no slow oracle."""
    import torch
    spec = synth.SynthSpec(200000, 4000, 8, paired=paired)
    dev = torch.device("cuda:0")
    t = synth.generate(spec, 0, spec.n_reads, device=dev)
    with ecb.EcBuilder(spec.n_loci, spec.n_haps) as b:
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        s = b.finalize()
        out = b.export()
    assert s["all_alignments"] == t["n_records"] and s["valid_alignments"] == t["n_valid"]
    assert s["n_reads"] == t["n_reads"] and int(out["dataN"].sum()) == t["n_reads"]
    with ecb.EcBuilder(spec.n_loci, spec.n_haps) as b:          # exactness pass: every read's set == its EC's key
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        assert b.verify_device(t["read_id"], t["locus"], t["hapflag"]) == (0, 0)
        assert b.finalize() == s                                 # the pass leaves the counters alone
        # ... and it does notice a read whose records no longer match the EC it was given
        hf2 = t["hapflag"].clone()
        i = int(torch.nonzero((hf2 & 0x4) == 0)[1000]) if not paired else int(torch.nonzero((hf2 & 0xC3) == 0x43)[1000])
        hf2[i] ^= (1 << 16)
        bad, _ = b.verify_device(t["read_id"], t["locus"], hf2)
        # (exactly that read: one haplotype bit of one valid record -- the checker on the read's records says whether its set changed)
        from verify_checker import misplaced
        rid = t["read_id"].cpu().numpy().view(np.uint32)
        a, z = np.searchsorted(rid, [rid[i], rid[i] + 1])
        one = {k: t[k][a:z].cpu().numpy().view(np.uint32) for k in ("locus", "hapflag")}
        one["read_id"] = np.zeros(z - a, np.uint32)
        assert int(misplaced(one, dict(one, hapflag=hf2[a:z].cpu().numpy().view(np.uint32)), spec.n_haps).sum()) == 1
        assert bad == 1
    assert np.all(np.diff(out["indptrA"]) > 0)
    for e in (0, 1, s["n_ecs"] // 2, s["n_ecs"] - 1):            # columns ascending within a row
        row = out["indicesA"][out["indptrA"][e]:out["indptrA"][e + 1]]
        assert np.all(np.diff(row) > 0)
    assert out["dataA"].min() >= 1 and out["dataA"].max() < (1 << spec.n_haps)
    # the same stream generated on the host gives the same answer through the host path
    th = synth.generate(spec, 0, spec.n_reads)
    assert np.array_equal(th["locus"].view(np.int32), t["locus"].cpu().numpy())
    out2, s2 = _run_host(th, spec.n_loci, spec.n_haps, batch=1 << 20)
    for k in ("indptrA", "indicesA", "dataA", "dataN"):
        assert np.array_equal(out[k], out2[k]), k


@pytest.mark.parametrize("stride,paired,paralogs", [(4, True, 0), (64, False, 0), (8, True, 0), (7, True, 0), (128, False, 30), (1, True, 30), (1, False, 60),
                                                    (1024, True, 100)])
def test_reads_whose_loci_collide_in_the_lds_table_match_the_c_oracle(stride, paired, paralogs, monkeypatch):
    """The stream kernel's LDS table gives a read a home region and places a locus in it by a fold of its bits (k_stream.inc: home_off): runs of
    consecutive target ids and loci a power of two apart do not meet there; loci seven apart do, and so do loci anywhere among the targets
    (`paralogs`: that percentage of the reads hit 1 - 3 further loci drawn uniformly, bench.py's c3r) at the birthday rate -- those records go
    through the probe-on rounds and their reads' lookups compare displaced pairs at their second place, or by the full key walk.
    600 k reads per case against the C oracle, bit for bit; the exactness pass agrees."""
    import torch
    from oracle import c_oracle
    spec = synth.SynthSpec(600_000, 20_000, 8, paired=paired, locus_stride=stride, paralog_pct=paralogs)
    dev = torch.device("cuda:0")
    t = synth.generate(spec, 0, spec.n_reads)
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], spec.n_haps, threads=4)
    d = [torch.from_numpy(t[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")]
    # (the stream kernel is compiled three times -- k_stream.inc: ks_std, ks_short, ks_par -- and the library picks per batch: every
    #  compilation a stream of this shape can take is forced in turn, and the library's own choice runs last, over a stream pushed in two
    #  batches so that the second one is picked by what the first one met)
    for force in ("ECB_NO_PAR", "ECB_FORCE_PAR", None):
        for k in ("ECB_NO_PAR", "ECB_FORCE_PAR"):
            monkeypatch.delenv(k, raising=False)
        if force:
            monkeypatch.setenv(force, "1")
        for hint in (0, exp["n_reads"]):
            with ecb.EcBuilder(spec.n_loci, spec.n_haps) as b:
                b.hint_reads(hint)
                if force is None:
                    rid, n = t["read_id"], len(t["read_id"])
                    cut = (n // 2) & ~3                     # (device streams must be 16-byte aligned: a multiple of four records)
                    while cut < n and rid[cut] == rid[cut - 1]:      # a record at which the run counter steps starts a read
                        cut += 4
                    assert 0 < cut < n
                    b.push_device(*[x[:cut] for x in d])
                    b.push_device(*[x[cut:] for x in d])
                    if paralogs >= 30 and hint:
                        assert b.profile_kernel().startswith("ks_par::"), b.profile_kernel()
                    if not paralogs and stride in (4, 8, 64, 1024):
                        assert b.profile_kernel().startswith("ks_std::"), b.profile_kernel()
                else:
                    b.push_device(*d)
                s = b.finalize()
                _check(b.export(), s, exp)
                b.reset()
                b.push_device(*d)
                assert b.verify_device(*d) == (0, 0)


def test_many_small_batches_do_not_leak_the_key_arena():
    """A stream pushed in hundreds of small host batches into a handle whose key arena is only ~2.5 x the keys it has to
    hold: a wave keeps the rest of its 512-pair reservation from launch to launch (leaving it behind per launch would
    overrun this arena after a few dozen batches).  Result == one push."""
    spec = synth.SynthSpec(40000, 3000, 8, paired=True)
    t = synth.generate(spec, 0, spec.n_reads)
    exp = _expect(t, spec.n_loci, spec.n_haps)
    nnz = int(exp["indptr"][-1])
    cap = 1 << 17
    assert nnz * 2 < cap < nnz * 4
    with ecb.EcBuilder(spec.n_loci, spec.n_haps, arena_capacity=cap, max_batch_records=4096) as b:
        b.push(t["read_id"], t["locus"], t["hapflag"])           # > 300 launches of a few waves each
        s = b.finalize()
        _check(b.export(), s, exp)


def test_shard_tables_merged_by_key_range_and_adopted():
    """The multi-GPU protocol of alntools_amd/dist.py without the collectives, on one GPU: three contiguous read shards,
    every table cut into three key ranges, range q of all shards merged (in shard order) into its own handle, the three
    merged ranges adopted by a root handle (tiny capacity: the adopt has to grow its table) == one handle over the
    whole stream, including EC order.  Also: the ranges hold every entry exactly once, and the states that must refuse."""
    import torch
    from alntools_amd import dist as ecdist
    spec = synth.SynthSpec(60000, 3000, 8, paired=True)
    dev = torch.device("cuda:0")
    whole = synth.generate(spec, 0, spec.n_reads)
    exp = _expect(whole, spec.n_loci, spec.n_haps)
    cuts = [0, 17000, 25000, spec.n_reads]
    P = 3
    pieces, sizes, base = [], [], 0
    for a, b_ in zip(cuts[:-1], cuts[1:]):
        t = synth.generate(spec, a, b_, device=dev)
        b = ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12)
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        eng = ecdist.GpuEngine(b, dev)
        ne, npairs, nreads = b.table_sizes()
        ent, prs, eoff, poff = eng.table_export_parts(base, P)
        assert eoff[0] == 0 and eoff[-1] == ne and poff[0] == 0 and all(x <= y for x, y in zip(eoff, eoff[1:]))
        e = ent[:ne * 4].view(-1, 4)
        assert int((e[:, 3] >> 32).sum()) == poff[-1]                    # every key pair exported once
        for q in range(P):                                               # offsets are relative to the part's pairs
            seg = e[eoff[q]:eoff[q + 1]]
            if len(seg):
                assert int(((seg[:, 3] & 0xFFFFFFFF) + (seg[:, 3] >> 32)).max()) <= poff[q + 1] - poff[q]
        pieces.append((ent, prs, eoff, poff))
        sizes.append((nreads,) + b.counters()[:2])
        base += nreads
        b.close()
    root = ecdist.GpuEngine(ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 10), dev)
    total = 0
    for q in range(P):
        part = ecdist.GpuEngine(ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12), dev)
        tabs = [(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                for ent, prs, eoff, poff in pieces if eoff[q + 1] > eoff[q]]
        if q == 0:
            for t in tabs:                                               # one by one ...
                part.table_merge(*t)
        else:
            part.table_merge_many(tabs)                                  # ... and as a batch (one host wait)
        pe_n, pp_n, _ = part.table_sizes()
        pe, pp = part.table_export(0)
        root.table_adopt(pe, pe_n, pp, pp_n)
        total += pe_n
        part.b.close()
    with pytest.raises(ecb.EcbError):
        root.table_merge(pe, pe_n, pp, pp_n)                             # no hashing into an adopted table
    with pytest.raises(ecb.EcbError):
        t = synth.generate(spec, 0, 10, device=dev)
        root.b.push_device(t["read_id"], t["locus"], t["hapflag"])
    root.add_counters(sum(s[1] for s in sizes), sum(s[2] for s in sizes), base)
    s = root.b.finalize()
    assert s["n_ecs"] == total
    out = root.b.export()
    _check(out, s, exp)
    assert s["n_reads"] == whole["n_reads"]
    root.b.close()
    built = ecb.EcBuilder(spec.n_loci, spec.n_haps)
    t = synth.generate(spec, 0, 100, device=dev)
    built.push_device(t["read_id"], t["locus"], t["hapflag"])
    with pytest.raises(ecb.EcbError):
        built.table_adopt_device(pe, pe_n, pp, pp_n)                     # adopt needs an empty handle
    built.close()


def test_shard_tables_merge_to_the_single_handle_result():
    """Two handles over contiguous read shards, tables exported / merged on one GPU (the multi-GPU protocol
    without the collective) == one handle over the whole stream, including EC order."""
    import torch
    from alntools_amd import dist as ecdist
    spec = synth.SynthSpec(60000, 3000, 8, paired=True)
    dev = torch.device("cuda:0")
    whole = synth.generate(spec, 0, spec.n_reads)
    exp = _expect(whole, spec.n_loci, spec.n_haps)
    cuts = [0, 25000, spec.n_reads]
    engines, sizes = [], []
    for a, b_ in zip(cuts[:-1], cuts[1:]):
        t = synth.generate(spec, a, b_, device=dev)
        b = ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12)
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        engines.append(ecdist.GpuEngine(b, dev))
        sizes.append(b.table_sizes() + b.counters()[:2])
    root = ecdist.GpuEngine(ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12), dev)
    base = 0
    for eng, (ne, npairs, nreads, n_all, n_valid) in zip(engines, sizes):
        ent, prs = eng.table_export(base)
        root.table_merge(ent, ne, prs, npairs)
        base += nreads
    root.add_counters(sum(s[3] for s in sizes), sum(s[4] for s in sizes), base)
    s = root.b.finalize()
    out = root.b.export()
    _check(out, s, exp)
    assert s["n_reads"] == whole["n_reads"]
    for e in engines + [root]:
        e.b.close()


def test_full_size_config3_properties():
    """BASELINE config 3 at full size (100 M paired-end reads, 3.3 G records -- record indices pass 2^31): properties
    that need no slow oracle.  Totals match the generator's own counts; the stream cut into two contiguous shards
    and merged by key range (the multi-GPU protocol on one card) gives the very same CSR (EC order included) as the whole."""
    import torch
    from alntools_amd import dist as ecdist
    sys_path_bench = os.path.join(os.path.dirname(__file__), "..")
    import sys
    sys.path.insert(0, sys_path_bench)
    import bench
    R, T, H, paired, _ = bench.WORKLOADS["c3"]
    spec = synth.SynthSpec(R, T, H, paired=paired)
    dev = torch.device("cuda:0")
    rid, loc, hf, st = bench.generate_shard(spec, 0, R, dev)
    assert st["records"] > (1 << 31)
    with ecb.EcBuilder(T, H, ec_capacity=1 << 24) as b:
        b.push_device(rid, loc, hf)
        s = b.finalize()
        whole = b.export()
    assert s["all_alignments"] == st["records"] and s["valid_alignments"] == st["valid"] and s["n_reads"] == st["reads"]
    _assert_equals_oracle(rid, loc, hf, H, whole, s)              # 3.7 M ECs in the reference's order, every row, every count
    assert int(whole["dataN"].astype(np.int64).sum()) == st["reads"]
    with ecb.EcBuilder(T, H, ec_capacity=1 << 24) as b:          # exact grouping at full size: 0 of 96 M reads differ
        b.push_device(rid, loc, hf)
        assert b.verify_device(rid, loc, hf) == (0, 0)
    assert np.all(np.diff(whole["indptrA"]) > 0) and whole["indptrA"][-1] == s["nnz_a"]
    assert whole["indicesA"].min() >= 0 and whole["indicesA"].max() < T
    assert whole["dataA"].min() >= 1 and whole["dataA"].max() < (1 << H)
    _assert_rows_distinct(whole, s["n_ecs"])
    rows = np.random.RandomState(1).randint(0, s["n_ecs"], 2000)
    for e in rows:
        r = whole["indicesA"][whole["indptrA"][e]:whole["indptrA"][e + 1]]
        assert np.all(np.diff(r) > 0)
    # two contiguous shards (cut on a read boundary well past 2^31 records), merged in order
    cut_read = int(st["reads"] * 0.7)
    cut = int(torch.searchsorted(rid, torch.tensor([cut_read], dtype=torch.int32, device=dev))[0])
    assert cut > (1 << 31)
    engines, meta = [], []
    for a, z, base in ((0, cut, 0), (cut, rid.numel(), cut_read)):
        bb = ecb.EcBuilder(T, H, ec_capacity=1 << 24)
        # the second shard keeps the global numbering of its read ids; libecb only needs them to continue from its first
        r2 = (rid[a:z] - base).contiguous() if base else rid[a:z]
        off = (16 - (a * 4) % 16) % 16          # device streams must be 16-byte aligned: copy the odd shard
        l2, h2 = loc[a:z], hf[a:z]
        if (a * 4) % 16:
            r2, l2, h2 = r2.clone(), l2.clone(), h2.clone()
        bb.push_device(r2, l2, h2)
        engines.append(ecdist.GpuEngine(bb, dev))
        meta.append(bb.table_sizes() + bb.counters()[:2])
    # ... by key range, as dist.py does across GPUs: cut both tables in two, merge range q of both, adopt the two results
    root = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 20), dev)     # (small: the adopt has to grow it)
    base, pieces = 0, []
    for eng, (ne, npairs, nreads, n_all, n_valid) in zip(engines, meta):
        pieces.append(eng.table_export_parts(base, 2))
        base += nreads
        eng.b.close()
    adopted = []
    for q in range(2):
        part = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 23), dev)
        part.table_merge_many([(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                               for ent, prs, eoff, poff in pieces])
        pe_n, pp_n, _ = part.table_sizes()
        adopted.append(part.table_export(0) + (pe_n, pp_n))
        part.b.close()
    del pieces
    root.table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
    root.add_counters(sum(m[3] for m in meta), sum(m[4] for m in meta), base)
    s2 = root.b.finalize()
    merged = root.b.export()
    assert s2 == s
    for k in ("indptrA", "indicesA", "dataA", "dataN"):
        assert np.array_equal(whole[k], merged[k]), k
    root.b.close()


def _assert_equals_oracle(rid, loc, hf, n_haps, out, s):
    """The whole stream through the oracle's C restatement (oracle/ec_oracle.c, all host threads) and the device's CSR A, counts and
    counters against it, bit for bit -- EC order (bam_utils.py:680-698) included, at BASELINE's full sizes."""
    from oracle import c_oracle
    host = [t.cpu().numpy().view(np.uint32) for t in (rid, loc, hf)]
    exp = c_oracle.ec_from_tuples(host[0], host[1], host[2], n_haps, threads=os.cpu_count() or 1)
    del host
    assert (s["all_alignments"], s["valid_alignments"], s["n_reads"], s["n_ecs"]) == (exp["n_all"], exp["n_valid"], exp["n_reads"], len(exp["count"]))
    for a, k in (("indptrA", "indptr"), ("indicesA", "indices"), ("dataA", "data"), ("dataN", "count")):
        assert np.array_equal(out[a], exp[k]), a


def _mix64(x, seed):
    with np.errstate(over="ignore"):
        x = x + np.uint64(seed)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _assert_rows_distinct(out, n_ecs):
    """No two ECs with the same key: two independent 64-bit hashes per CSR row -- the sum over the row of a splitmix64 of
    (locus, mask, position); columns are ascending, so equal rows hash equal, and unequal rows do with probability ~2^-128."""
    ip = out["indptrA"].astype(np.int64)
    v = (out["indicesA"].astype(np.uint64) << np.uint64(32)) | out["dataA"].astype(np.uint64)
    pos = np.arange(len(v), dtype=np.uint64) - np.repeat(ip[:-1], np.diff(ip)).astype(np.uint64)
    with np.errstate(over="ignore"):
        h1 = np.add.reduceat(_mix64(v ^ _mix64(pos, 0x9E3779B97F4A7C15), 1), ip[:-1])
        h2 = np.add.reduceat(_mix64(v + _mix64(pos, 0xD6E8FEB86659FD93), 0xC2B2AE3D27D4EB4F), ip[:-1])
    both = np.stack([h1, h2, np.diff(ip).astype(np.uint64)], axis=1)
    assert len(np.unique(both, axis=0)) == n_ecs, "two equivalence classes with the same target set"


def test_full_size_config2_properties():
    """BASELINE config 2 at full size (50 M single-end reads, 8 haplotypes x 40 k transcripts): totals against the generator's
    own counts, the independent exactness pass over all 48 M reads, distinct EC keys, CSR invariants."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench
    R, T, H, paired, _ = bench.WORKLOADS["c2"]
    spec = synth.SynthSpec(R, T, H, paired=paired)
    dev = torch.device("cuda:0")
    rid, loc, hf, st = bench.generate_shard(spec, 0, R, dev)
    with ecb.EcBuilder(T, H, ec_capacity=1 << 22) as b:
        b.push_device(rid, loc, hf)
        assert b.verify_device(rid, loc, hf) == (0, 0)            # every read's target set == the key of its EC
        s = b.finalize()
        out = b.export()
    assert s["all_alignments"] == st["records"] and s["valid_alignments"] == st["valid"] and s["n_reads"] == st["reads"]
    _assert_equals_oracle(rid, loc, hf, H, out, s)
    assert int(out["dataN"].astype(np.int64).sum()) == st["reads"] and out["dataN"].min() >= 1
    assert np.all(np.diff(out["indptrA"]) > 0) and out["indptrA"][-1] == s["nnz_a"]
    assert out["indicesA"].min() >= 0 and out["indicesA"].max() < T and out["dataA"].min() >= 1 and out["dataA"].max() < (1 << H)
    inner = np.ones(len(out["indicesA"]), dtype=bool)
    inner[out["indptrA"][:-1]] = False
    assert np.all(np.diff(out["indicesA"].astype(np.int64))[inner[1:]] > 0)          # columns ascending within every row
    _assert_rows_distinct(out, s["n_ecs"])


def test_full_size_config4_multisample_triples():
    """BASELINE config 4 at full size on one GPU: 200 M paired-end reads, 5 000 cell barcodes, 64 files.  The EC of every read
    is checked by the independent exactness pass (re-derived from the records, compared with the stored key: 0 of 192 M
    differ), so the per-read EC ranks are a sound basis: the (EC, cell, file) triples, their counts and first reads must be
    exactly the groups of (rank, meta) over the reads."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench
    R, T, H = 200_000_000, 80_000, 8
    spec = synth.SynthSpec(R, T, H, paired=True)
    dev = torch.device("cuda:0")
    rid, loc, hf, st = bench.generate_shard(spec, 0, R, dev)
    n_reads = st["reads"]
    g = torch.arange(n_reads, dtype=torch.int64, device=dev)
    x = ((g * 0x9E3779B97F4A7C15) >> 20) & 0x7FFFFFFFFFF
    cell = x % 5000
    cell = torch.where((x % 7) == 0, torch.full_like(cell, 17), cell)           # one big cell
    fil = (g * 64) // n_reads                                                     # 64 files: contiguous read ranges, as a directory scan gives
    meta = (cell | (fil << 22)).to(torch.int32)
    with ecb.EcBuilder(T, H, multisample=True, ec_capacity=1 << 24) as b:
        b.push_device(rid, loc, hf)
        assert b.verify_device(rid, loc, hf) == (0, 0)
        del loc, hf
        b.push_cells(meta.cpu().numpy().view(np.uint32), 0)
        s = b.finalize()
        pr = b.export_pairs()
        rec = torch.from_numpy(b.export_read_ec()).to(dev)
        a = b.export()
        f = b.ms_filter(5000, 1000)                                               # config 4's minimum count
    assert s["n_reads"] == n_reads and int(pr["count"].sum()) == n_reads
    # cell order, filter, EC re-rank, CSC N and the surviving rows of A at config 4's size, against the numpy restatement that
    # tests/test_oracle_golden.py holds to the reference's bytes
    from ms_checker import reduce_triples, select_rows
    kept, ec_keep, (n_ptr, n_idx, n_dat) = reduce_triples(pr, s["n_ecs"], 5000, 1000)
    a_ptr, a_idx, a_dat = select_rows(a["indptrA"], a["indicesA"], a["dataA"], ec_keep)
    assert f["kept_cells"].tolist() == kept and 0 < len(kept) <= 5000
    for k, exp in (("indptrA", a_ptr), ("indicesA", a_idx), ("dataA", a_dat), ("indptrN", n_ptr), ("indicesN", n_idx), ("dataN", n_dat)):
        assert np.array_equal(f[k], exp), k
    del a, f, kept, ec_keep, n_ptr, n_idx, n_dat, a_ptr, a_idx, a_dat
    m64 = meta.to(torch.int64) & 0xFFFFFFFF
    key = (rec.to(torch.int64) << 32) | ((m64 & 0x3FFFFF) << 10) | (m64 >> 22)    # the triples come sorted by (EC, cell, file)
    order = torch.argsort(key, stable=True)
    ks = key[order]
    heads = torch.nonzero(torch.cat([torch.ones(1, dtype=torch.bool, device=dev), ks[1:] != ks[:-1]])).flatten()
    exp_key = ks[heads].cpu().numpy()
    exp_cnt = torch.diff(torch.cat([heads, torch.tensor([len(ks)], device=dev)])).cpu().numpy()
    exp_first = order[heads].cpu().numpy()                                        # stable sort: a run starts with its smallest read
    got_key = (pr["ec"] << 32) | (pr["cell"] << 10) | pr["file"]
    assert len(got_key) == len(exp_key) == s["nnz_n"]
    assert np.array_equal(got_key, exp_key) and np.array_equal(pr["count"], exp_cnt) and np.array_equal(pr["first"], exp_first)


def test_full_size_config5_round_trip_and_ranges():
    """BASELINE config 5 on config 3's output: (i) CSR(bitmask) -> per-haplotype CSC -> CSR on the 12 M-nnz matrix of the
    100 M-read stream gives the same arrays back, every set bit exactly once; (ii) the range reduction over all 3.3 G
    records equals torch's own min / max per (locus, haplotype)."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench
    R, T, H, paired, _ = bench.WORKLOADS["c3"]
    spec = synth.SynthSpec(R, T, H, paired=paired)
    dev = torch.device("cuda:0")
    rid, loc, hf, st = bench.generate_shard(spec, 0, R, dev)
    n = rid.numel()
    pos = ((torch.arange(n, dtype=torch.int64, device=dev) * 1103515245 + 12345) % 4999).to(torch.int32)
    with ecb.EcBuilder(T, H, ec_capacity=1 << 24, track_ranges=True) as b:
        b.push_device(rid, loc, hf, pos)
        s = b.finalize()
        out = b.export()
        rng = b.export_ranges()
    del rid
    # (ii) ranges: max - min + 1 over the valid records of every (locus, haplotype), 0 where none
    lo = torch.full((T * H,), 1 << 40, dtype=torch.int64, device=dev)
    hi = torch.full((T * H,), -1, dtype=torch.int64, device=dev)
    for c0 in range(0, n, 1 << 29):                                   # (in pieces: torch indexes with 32 bits)
        c1 = min(c0 + (1 << 29), n)
        f = hf[c0:c1].to(torch.int64) & 0xFFFFFFFF
        valid = ((f & 4) == 0) & (((f & 1) == 0) | (((f ^ 2) & 0x3082) == 0))
        slot = (loc[c0:c1].to(torch.int64) * H + ((f >> 16) & 0xFF))[valid]
        pv = pos[c0:c1].to(torch.int64)[valid]
        lo.scatter_reduce_(0, slot, pv, "amin")
        hi.scatter_reduce_(0, slot, pv, "amax")
    exp = torch.where(hi >= 0, hi - lo + 1, torch.zeros_like(hi)).cpu().numpy().reshape(T, H)
    assert np.array_equal(rng, exp)
    del f, valid, slot, pv, loc, hf, pos
    # (i) the sparse-format round trip at full size
    ip, ix, da = (torch.from_numpy(out[k]).to(dev) for k in ("indptrA", "indicesA", "dataA"))
    cptr, cidx = ecb.csr_to_hapcsc(ip, ix, da, T, H)
    bits = int(sum(int(((out["dataA"] >> h) & 1).sum()) for h in range(H)))
    assert cidx.numel() == bits and int(cptr[:, -1].sum()) == bits
    # two haplotypes' matrices against scipy's own CSR -> CSC of the same bit plane (what ec2emase stores, bin_utils.py:324-335), at full size
    import scipy.sparse as sp
    cp, ci = cptr.cpu().numpy(), cidx.cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(cp[:, -1].astype(np.int64))])
    for h in (0, H - 1):
        keep = ((out["dataA"] >> h) & 1).astype(bool)
        rows = np.repeat(np.arange(s["n_ecs"], dtype=np.int32), np.diff(out["indptrA"]))[keep]
        m = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows, out["indicesA"][keep])), shape=(s["n_ecs"], T)).tocsc()
        m.sort_indices()
        assert np.array_equal(cp[h], m.indptr) and np.array_equal(ci[starts[h]:starts[h + 1]], m.indices), h
    del cp, ci, m, rows, keep
    ip2, ix2, da2 = ecb.hapcsc_to_csr(cptr, cidx, s["n_ecs"])
    assert torch.equal(ip2, ip) and torch.equal(ix2, ix) and torch.equal(da2, da)
    _assert_rows_distinct(out, s["n_ecs"])


def test_sparse_format_round_trip_on_device(golden_dir):
    """f-2 / BASELINE config 5: CSR(bitmask) -> per-haplotype CSC -> CSR on the device; per-haplotype CSC equals scipy's
    (what ec2emase stores), and the round trip reproduces the .bin arrays exactly."""
    import torch
    from alntools_amd import bin_utils
    dev = torch.device("cuda:0")
    for name in ("g2_c1.bin", "g1_edge.bin", "g4_multi_min0.bin"):
        m = bin_utils.ecload(os.path.join(golden_dir, name))
        ip, ix, da = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (m.indptrA, m.indicesA, m.dataA))
        cptr, cidx = ecb.csr_to_hapcsc(ip, ix, da, m.num_loci, m.num_haplotypes)
        cptr_h, cidx_h = cptr.cpu().numpy(), cidx.cpu().numpy()
        start = 0
        for h in range(m.num_haplotypes):
            ref = m.haplotype_csc(h)
            assert np.array_equal(cptr_h[h], ref.indptr), (name, h)
            assert np.array_equal(cidx_h[start:start + ref.nnz], ref.indices), (name, h)
            start += ref.nnz
        ip2, ix2, da2 = ecb.hapcsc_to_csr(cptr, cidx, m.num_reads)
        assert np.array_equal(ip2.cpu().numpy(), m.indptrA) and np.array_equal(ix2.cpu().numpy(), m.indicesA)
        assert np.array_equal(da2.cpu().numpy(), m.dataA)


def test_sparse_format_conversion_refuses_a_malformed_matrix(golden_dir):
    """``ecb_csr_to_hapcsc_device`` takes matrices of unknown origin (``ec2emase`` of a ``.bin`` from disk): a locus beyond n_loci, a
    mask that is zero or has a bit beyond the haplotypes, row pointers out of order -- ECB_ERR_CONTRACT, nothing written past a buffer;
    the count-only first call of the C ABI (NULL outputs) still gives the number of set bits; 31 haplotypes, empty rows and a matrix
    without non-zeros go through."""
    import ctypes as C
    import torch
    from alntools_amd import bin_utils
    dev = torch.device("cuda:0")
    m = bin_utils.ecload(os.path.join(golden_dir, "g2_c1.bin"))
    good = [np.ascontiguousarray(a).astype(np.int32) for a in (m.indptrA, m.indicesA, m.dataA)]
    T, H = m.num_loci, m.num_haplotypes

    def run(ip, ix, da, T=T, H=H):
        return ecb.csr_to_hapcsc(*(torch.from_numpy(a).to(dev) for a in (ip, ix, da)), T, H)

    cptr, cidx = run(*good)
    bits = int(sum(int(((good[2] >> h) & 1).sum()) for h in range(H)))
    assert cidx.numel() == bits
    lib, tot = ecb.load(), C.c_uint64()
    t = [torch.from_numpy(a).to(dev) for a in good]
    assert lib.ecb_csr_to_hapcsc_device(0, len(good[0]) - 1, T, H, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()),
                                        C.c_void_p(t[2].data_ptr()), None, None, C.byref(tot)) == 0 and tot.value == bits
    for what in ("locus", "zero mask", "wide mask", "pointers"):
        ip, ix, da = (a.copy() for a in good)
        if what == "locus":
            ix[len(ix) // 2] = T
        elif what == "zero mask":
            da[3] = 0
        elif what == "wide mask":
            da[5] = 1 << H
        else:
            ip[7], ip[8] = ip[8], ip[7] - 1
        with pytest.raises(ecb.EcbError) as e:
            run(ip, ix, da)
        assert e.value.code == -5, what
    # 31 haplotypes (bit 30), rows without entries, one column used by every row
    ip = np.array([0, 2, 2, 3, 3, 5], dtype=np.int32)
    ix = np.array([1, 4, 4, 0, 4], dtype=np.int32)
    da = np.array([1 << 30, 3, (1 << 30) | 1, 7, 1 << 29], dtype=np.int32)
    cptr, cidx = run(ip, ix, da, T=6, H=31)
    cp, ci = cptr.cpu().numpy(), cidx.cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(cp[:, -1])])
    for h, exp in ((30, {1: [0], 4: [2]}), (0, {4: [0, 2], 0: [4]}), (29, {4: [4]}), (5, {})):
        for tcol in range(6):
            got = ci[starts[h] + cp[h, tcol]:starts[h] + cp[h, tcol + 1]].tolist()
            assert got == exp.get(tcol, []), (h, tcol)
    cptr, cidx = run(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), T=5, H=2)
    assert cidx.numel() == 0 and int(cptr.abs().sum()) == 0
    assert lib.ecb_release_scratch(0) == 0


def test_per_haplotype_csc_of_any_origin_converts_back(golden_dir):
    """``ecb_hapcsc_to_csr_device`` (``emase2ec`` of an ``.h5`` from disk): lists in scipy's canonical order take the union-and-transpose
    path; lists whose rows are out of order, or hold an EC twice, are noticed and sorted -- the same CSR either way; column pointers
    that go backwards and a row index beyond the ECs are ECB_ERR_CONTRACT; columns without entries, haplotypes without entries, one
    column that every EC uses and lists far longer than a workgroup's stretch go through."""
    import torch
    from alntools_amd import bin_utils
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    m = bin_utils.ecload(os.path.join(golden_dir, "g2_c1.bin"))
    T, H, E = m.num_loci, m.num_haplotypes, m.num_reads
    ip, ix, da = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (m.indptrA, m.indicesA, m.dataA))
    cptr, cidx = ecb.csr_to_hapcsc(ip, ix, da, T, H)
    cp, ci = cptr.cpu().numpy().copy(), cidx.cpu().numpy().copy()
    starts = np.concatenate([[0], np.cumsum(cp[:, -1])]).astype(np.int64)

    def back(cp_, ci_, n_ecs=E):
        a, b, c = ecb.hapcsc_to_csr(torch.from_numpy(cp_).to(dev), torch.from_numpy(ci_).to(dev), n_ecs)
        return a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()

    def same(got):
        return np.array_equal(got[0], m.indptrA) and np.array_equal(got[1], m.indicesA) and np.array_equal(got[2], m.dataA)

    assert same(back(cp, ci))
    # every list shuffled: the general path
    sh = ci.copy()
    for h in range(H):
        for t in range(T):
            a, b = starts[h] + cp[h, t], starts[h] + cp[h, t + 1]
            if b - a > 1:
                sh[a:b] = rng.permutation(sh[a:b])
    assert not np.array_equal(sh, ci) and same(back(cp, sh))
    # an EC twice in a list (a duplicate entry ORs into the same bit): one list gets its first row index once more
    h0, t0 = next((h, t) for h in range(H) for t in range(T) if cp[h, t + 1] > cp[h, t])
    at = int(starts[h0] + cp[h0, t0])
    dup_ci = np.concatenate([ci[:at], ci[at:at + 1], ci[at:]])
    dup_cp = cp.copy()
    dup_cp[h0, t0 + 1:] += 1
    assert same(back(dup_cp, dup_ci))
    for what in ("pointers", "row index"):
        cp2, ci2 = cp.copy(), ci.copy()
        if what == "pointers":
            cp2[1, 5], cp2[1, 6] = cp2[1, 6] + 1, cp2[1, 5]
        else:
            ci2[len(ci2) // 3] = E
        with pytest.raises(ecb.EcbError) as e:
            back(cp2, ci2)
        assert e.value.code == -5, what
    # a made-up matrix: 3 000 ECs x 40 loci x 5 haplotypes, haplotype 3 empty, loci 7 - 19 unused, locus 2 in every EC on haplotype 0
    # and 1 (two lists of 3 000 rows: a dozen workgroups' stretches each), the rest sparse
    E2, T2, H2 = 3000, 40, 5
    dense = np.zeros((E2, T2), dtype=np.int32)
    dense[:, 2] = 3
    for h in (0, 1, 2, 4):
        r, c = rng.integers(0, E2, 4000), rng.integers(20, T2, 4000)
        dense[r, c] |= 1 << h
    from scipy import sparse
    ref = sparse.csr_matrix(dense)
    ref.sort_indices()
    cps, cis = [], []
    for h in range(H2):
        mh = sparse.csc_matrix((dense >> h) & 1)
        mh.sort_indices()
        cps.append(mh.indptr.astype(np.int32)); cis.append(mh.indices.astype(np.int32))
    g = back(np.stack(cps), np.concatenate(cis), E2)
    assert np.array_equal(g[0], ref.indptr) and np.array_equal(g[1], ref.indices) and np.array_equal(g[2], ref.data)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_per_haplotype_csc_with_long_and_bunched_columns(seed):
    """The union-per-column path of ``ecb_hapcsc_to_csr_device`` on shapes that stress its cuts: a column far longer than a piece of
    work whose ECs are spread over all ids (cut into EC ranges, hashed in LDS), one whose ECs are bunched into a narrow range (one piece
    overflows its table: the entry-by-entry path with binary searches), up to 31 haplotypes, empty haplotypes and columns; and the same
    matrix with the long columns' lists shuffled (noticed; the sort-everything path).  Against scipy."""
    import torch
    from scipy import sparse
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 + seed)
    E, T, H = (200_000, 30, 4) if seed == 1 else ((90_000, 12, 31) if seed == 2 else (400_000, 200, 8))
    rows, cols, bits = [], [], []

    def add(r, c, h):
        rows.append(np.asarray(r, dtype=np.int64)); cols.append(np.full(len(r), c, dtype=np.int64)); bits.append(np.full(len(r), h, dtype=np.int64))
    for h in range(H):
        if h == 1:
            continue                                                   # a haplotype without entries
        add(rng.choice(E, size=min(E, 20_000), replace=False), 0, h)   # long, spread over all ids
        add(rng.choice(5_000, size=4_000, replace=False), 1, h)        # long, bunched at low ids
        for c in range(3, T):                                          # (column 2 stays empty)
            add(rng.choice(E, size=int(rng.integers(0, 60)), replace=False), c, h)
    r, c, b = np.concatenate(rows), np.concatenate(cols), np.concatenate(bits)
    ref = sparse.coo_matrix(((1 << b).astype(np.int64), (r, c)), shape=(E, T)).tocsr()      # (distinct bits per (row, column, haplotype): the sum is the OR)
    ref.sort_indices()
    cps, cis = [], []
    for h in range(H):
        sel = b == h
        mh = sparse.coo_matrix((np.ones(int(sel.sum()), dtype=np.int8), (r[sel], c[sel])), shape=(E, T)).tocsc()
        mh.sort_indices()
        cps.append(mh.indptr.astype(np.int32)); cis.append(mh.indices.astype(np.int32))
    cp, ci = np.stack(cps), np.concatenate(cis)

    def back(ci_):
        a, x, d = ecb.hapcsc_to_csr(torch.from_numpy(cp).to(dev), torch.from_numpy(ci_).to(dev), E)
        return a.cpu().numpy(), x.cpu().numpy(), d.cpu().numpy()

    def same(g):
        return np.array_equal(g[0], ref.indptr) and np.array_equal(g[1], ref.indices) and np.array_equal(g[2], ref.data.astype(np.int32))

    assert same(back(ci))
    starts = np.concatenate([[0], np.cumsum(cp[:, -1])]).astype(np.int64)
    sh = ci.copy()
    for h in range(H):
        for col in (0, 1):
            a, e = starts[h] + cp[h, col], starts[h] + cp[h, col + 1]
            if e - a > 1:
                sh[a:e] = rng.permutation(sh[a:e])
    assert same(back(sh))
    # ... and forward again: the per-haplotype CSC of the CSR is the one it came from
    cptr, cidx = ecb.csr_to_hapcsc(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ref.indptr.astype(np.int32), ref.indices.astype(np.int32), ref.data.astype(np.int32))), T, H)
    assert np.array_equal(cptr.cpu().numpy(), cp) and np.array_equal(cidx.cpu().numpy(), ci)


def test_cells_pushed_from_device_memory_equal_cells_pushed_from_the_host():
    import torch
    spec = synth.SynthSpec(50_000, 3_000, 4)
    dev = torch.device("cuda:0")
    t = synth.generate(spec, 0, spec.n_reads, device=dev)
    g = np.arange(t["n_reads"], dtype=np.uint64)
    meta = (((g * np.uint64(2654435761)) % np.uint64(97)) | ((g * np.uint64(3) // np.uint64(t["n_reads"])) << np.uint64(22))).astype(np.uint32)
    res = []
    for device_side in (False, True):
        with ecb.EcBuilder(spec.n_loci, spec.n_haps, multisample=True) as b:
            b.push_device(t["read_id"], t["locus"], t["hapflag"])
            if device_side:
                half = len(meta) // 2                                                 # in two pieces, the second first
                m_dev = torch.from_numpy(meta.view(np.int32)).to(dev)
                b.push_cells_device(m_dev[half:], half)
                b.push_cells_device(m_dev[:half], 0)
            else:
                b.push_cells(meta, 0)
            b.finalize()
            res.append((b.export_pairs(), b.ms_filter(97, 300)))
    for k in ("ec", "cell", "file", "count", "first"):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for k in ("kept_cells", "indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN"):
        assert np.array_equal(res[0][1][k], res[1][1][k]), k


def test_sparse_format_round_trip_at_scale():
    import torch
    spec = synth.SynthSpec(3_000_000, 40_000, 8, paired=True)
    dev = torch.device("cuda:0")
    t = synth.generate(spec, 0, spec.n_reads, device=dev)
    with ecb.EcBuilder(spec.n_loci, spec.n_haps) as b:
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        s = b.finalize()
        out = b.export()
    ip, ix, da = (torch.from_numpy(out[k]).to(dev) for k in ("indptrA", "indicesA", "dataA"))
    cptr, cidx = ecb.csr_to_hapcsc(ip, ix, da, spec.n_loci, spec.n_haps)
    assert cidx.numel() == int(np.unpackbits(out["dataA"].astype(np.uint8)).sum())      # one entry per set haplotype bit
    rows = cidx.cpu().numpy()
    ptr = cptr.cpu().numpy().astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(ptr[:, -1])])
    for h in (0, spec.n_haps - 1):                                                       # rows ascending within every column
        seg = rows[starts[h]:starts[h + 1]]
        brk = np.zeros(len(seg), dtype=bool)
        brk[ptr[h][1:-1][ptr[h][1:-1] < len(seg)]] = True
        d = np.diff(seg)
        assert np.all((d > 0) | brk[1:])
    ip2, ix2, da2 = ecb.hapcsc_to_csr(cptr, cidx, s["n_ecs"])
    assert torch.equal(ip2, ip) and torch.equal(ix2, ix) and torch.equal(da2, da)


def _random_stream(seed, n_reads, n_loci, n_haps, max_len, p_invalid, loci_mode):
    """Unstructured tuples: random read lengths, loci drawn to collide in the LDS tables, duplicate records,
    invalid records anywhere (also first and last), every haplotype index up to n_haps - 1."""
    rng = np.random.RandomState(seed)
    rid, loc, hf = [], [], []
    cur = -1
    for _ in range(n_reads):
        L = int(rng.randint(1, max_len + 1))
        if loci_mode == "strided":            # congruent low bits: worst case for the low-bit probe start
            pool = (rng.randint(0, max(n_loci // 64, 1)) * 64 + 64 * np.arange(8)) % n_loci
        elif loci_mode == "wide":
            pool = rng.randint(0, n_loci, size=max(L, 1))
        else:
            base = rng.randint(0, n_loci)
            pool = (base + np.arange(4)) % n_loci
        started = False
        for _ in range(L):
            valid = rng.rand() >= p_invalid
            if valid and not started:
                cur += 1
                started = True
            flag = 0x10 if rng.rand() < 0.5 else 0
            if not valid:
                flag = 0x4 if rng.rand() < 0.5 else (0x1 | 0x40)          # unmapped, or paired but not proper
            rid.append(cur if cur >= 0 else 0xFFFFFFFF)
            loc.append(int(pool[rng.randint(len(pool))]))
            hf.append(flag | (int(rng.randint(n_haps)) << 16))
    return dict(read_id=np.array(rid, dtype=np.uint64).astype(np.uint32), locus=np.array(loc, dtype=np.uint32),
                hapflag=np.array(hf, dtype=np.uint32), pos=np.zeros(len(rid), np.int32))


@pytest.mark.parametrize("seed,n_loci,n_haps,max_len,p_inv,mode", [
    (1, 50, 1, 60, 0.1, "wide"),                 # one haplotype: every record a new locus, tables at their fullest
    (2, 1 << 20, 31, 40, 0.2, "strided"),        # 31 haplotypes (bit 30 set), loci congruent mod 64
    (3, (1 << 26) - 3, 8, 200, 0.05, "wide"),    # the largest locus index the key packing allows; long reads (carried over tiles, some via k_slow)
    (4, 300, 4, 12, 0.5, "near"),                # half the records invalid
    (5, 7, 2, 3, 0.0, "near"),                   # tiny reads: more than 64 reads per tile
])
def test_random_streams_match_the_c_oracle(seed, n_loci, n_haps, max_len, p_inv, mode):
    from oracle import c_oracle
    t = _random_stream(seed, 6000, n_loci, n_haps, max_len, p_inv, mode)
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], n_haps, threads=2)
    for batch in (None, 777):
        out, sizes = _run_host(t, n_loci, n_haps, batch=batch)
        _check(out, sizes, exp)
        assert sizes["n_reads"] == exp["n_reads"]


@pytest.mark.parametrize("seed,n_loci,n_haps,max_len,p_inv,mode", [
    (11, 7, 2, 3, 0.0, "near"),                   # what the kernel is for: a few records per read, 200 reads per tile
    (12, 40_000, 2, 6, 0.1, "near"),              # diploid, consecutive loci
    (13, (1 << 25) - 3, 8, 9, 0.3, "wide"),       # the largest locus its keys hold
    (14, 50, 1, 60, 0.1, "wide"),                 # forced onto it: long reads (carried over tiles), full tables
    (15, 1 << 20, 31, 200, 0.2, "strided"),       # forced: 31 haplotypes, colliding loci, reads beyond the carry limit (k_slow)
])
def test_short_read_kernel_matches_the_c_oracle(seed, n_loci, n_haps, max_len, p_inv, mode, monkeypatch):
    """``ks_short::k_stream`` (passes of up to 128 reads, looked up 64 at a time over one LDS table; chosen when the caller has bounded the
    stream's reads and a batch brings fewer than seven records per read): the same CSR as the oracle's, in one device push and in several,
    with a table that has to grow, and for streams it is not meant for (forced by ECB_FORCE_SHORT); ECB_NO_SHORT gives the standard
    kernel the same input; the exactness pass agrees."""
    import torch
    from oracle import c_oracle
    dev = torch.device("cuda:0")
    t = _random_stream(seed, 20000 if max_len <= 9 else 3000, n_loci, n_haps, max_len, p_inv, mode)
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], n_haps, threads=2)
    d = [torch.from_numpy(t[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")]
    n = len(t["read_id"])
    cuts = [0]
    for frac in (0.37, 0.7, 1.0):
        c = min(int(n * frac), n)
        while 0 < c < n and t["read_id"][c] == t["read_id"][c - 1]:
            c += 1
        cuts.append(c)
    for env in ({"ECB_FORCE_SHORT": "1"}, {"ECB_NO_SHORT": "1"}):
        for k in ("ECB_FORCE_SHORT", "ECB_NO_SHORT"):
            monkeypatch.delenv(k, raising=False)
        if max_len > 9 or "ECB_NO_SHORT" in env:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
        for kw in ({}, {"ec_capacity": 256}):
            with ecb.EcBuilder(n_loci, n_haps, **kw) as b:
                b.hint_reads(exp["n_reads"])
                b.push_device(*d)
                s = b.finalize()
                _check(b.export(), s, exp)
                assert s["n_reads"] == exp["n_reads"]
                b.reset()
                for a, e in zip(cuts[:-1], cuts[1:]):
                    if e > a:
                        b.push_device(*(x[a:e].clone() for x in d))
                s = b.finalize()
                _check(b.export(), s, exp)
                b.reset()
                b.push_device(*d)
                bad, _ = b.verify_device(*d)
                assert bad == 0
    # its haplotype masks are bytes: an index beyond 7 in a valid record must be refused before it can reach a neighbour's byte
    if n_haps == 8:
        for k in ("ECB_FORCE_SHORT", "ECB_NO_SHORT"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("ECB_FORCE_SHORT", "1")
        hf = t["hapflag"].copy()
        ok = np.where((hf & 0x4) == 0)[0]
        hf[ok[len(ok) // 2]] = (hf[ok[len(ok) // 2]] & 0xFFFF) | (11 << 16)
        with ecb.EcBuilder(n_loci, n_haps) as b:
            b.hint_reads(exp["n_reads"])
            with pytest.raises(ecb.EcbError) as e:
                b.push_device(d[0], d[1], torch.from_numpy(hf.view(np.int32)).to(dev))
                b.finalize()
            assert e.value.code == -5


def test_multisample_triples_at_scale():
    """BASELINE config 4's shape on one GPU, scaled to 20 M paired-end reads: 5 000 cell barcodes over 3 files, per-(EC, cell,
    file) counts.  The device's triple reduce (radix sort + run lengths over 19 M reads) is checked against numpy on the
    per-read EC ranks the same handle exports: same triples, same counts, same first reads; the counts add up to the reads."""
    import torch
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench
    R, T, H = 20_000_000, 80_000, 8
    spec = synth.SynthSpec(R, T, H, paired=True)
    dev = torch.device("cuda:0")
    rid, loc, hf, st = bench.generate_shard(spec, 0, R, dev)
    n_reads = st["reads"]
    x = (np.arange(n_reads, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(20)
    cell = (x % np.uint64(5000)).astype(np.uint32)
    cell[(x % np.uint64(7)) == 0] = 17                      # one big cell
    fil = ((x >> np.uint64(13)) % np.uint64(3)).astype(np.uint32)
    meta = cell | (fil << np.uint32(22))
    with ecb.EcBuilder(T, H, multisample=True, ec_capacity=1 << 22) as b:
        b.push_device(rid, loc, hf)
        b.push_cells(meta, 0)
        s = b.finalize()
        pr = b.export_pairs()
        rec = b.export_read_ec()
    assert s["n_reads"] == n_reads and len(rec) == n_reads
    assert rec.min() == 0 and rec.max() == s["n_ecs"] - 1
    assert int(pr["count"].sum()) == n_reads
    m64 = meta.astype(np.int64)
    key = (rec.astype(np.int64) << 32) | ((m64 & 0x3FFFFF) << 10) | (m64 >> 22)   # the triples come sorted by (EC, cell, file)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    exp_key, exp_cnt = ks[heads], np.diff(np.concatenate((heads, [len(ks)])))
    exp_first = order[heads]                                # stable sort: the first of a run is its smallest read index
    got_key = (pr["ec"] << 32) | (pr["cell"] << 10) | pr["file"]
    assert len(got_key) == len(exp_key) == s["nnz_n"]
    assert np.array_equal(got_key, exp_key)
    assert np.array_equal(pr["count"], exp_cnt)
    assert np.array_equal(pr["first"], exp_first)


@pytest.mark.parametrize("mincount", [-1, "median", "p90", 10**7])
def test_multisample_filter_on_device_matches_the_numpy_checker(mincount):
    """K4' / K5' (bam_utils_multisample.py:596-636, 737-791) on the device -- cell order, minimum-count filter, EC re-rank,
    CSC N, surviving rows of A -- against the numpy restatement of the same reduction (tests/ms_checker.py) on the triples
    the handle exports: 6 M reads, 1 500 cells whose reads are spread over 3 files, thresholds that keep all, most, few and
    none of the cells."""
    import torch
    from ms_checker import reduce_triples, select_rows
    R, T, H = 6_000_000, 20_000, 8
    spec = synth.SynthSpec(R, T, H, paired=True)
    dev = torch.device("cuda:0")
    t = synth.generate(spec, 0, R, device=dev)
    n_reads = t["n_reads"]
    x = (np.arange(n_reads, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(20)
    cell = ((x % np.uint64(1500)) * (x % np.uint64(1500)) // np.uint64(1500)).astype(np.uint32)      # skewed cell sizes
    fil = (np.arange(n_reads, dtype=np.uint64) * np.uint64(3) // np.uint64(n_reads)).astype(np.uint32)   # 3 files, contiguous
    # cell ids are handed out in order of first appearance, as convert_files does
    _, first_idx, inv = np.unique(cell, return_index=True, return_inverse=True)
    rank = np.empty(len(first_idx), dtype=np.uint32)
    rank[np.argsort(first_idx)] = np.arange(len(first_idx), dtype=np.uint32)
    cell = rank[inv]
    n_cells = int(cell.max()) + 1
    if isinstance(mincount, str):                                    # a threshold that keeps half / a tenth of the cells
        mincount = int(np.quantile(np.bincount(cell), 0.5 if mincount == "median" else 0.9)) + 1
    with ecb.EcBuilder(T, H, multisample=True, ec_capacity=1 << 21) as b:
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        b.push_cells(cell | (fil << np.uint32(22)), 0)
        s = b.finalize()
        a = b.export()
        tr = b.export_pairs()
        if mincount == 10**7:
            with pytest.raises(ecb.EcbError) as e:
                b.ms_filter(n_cells, mincount)
            assert e.value.code == -7
            return
        f = b.ms_filter(n_cells, mincount)
    kept, ec_keep, (n_ptr, n_idx, n_dat) = reduce_triples(tr, s["n_ecs"], n_cells, mincount)
    a_ptr, a_idx, a_dat = select_rows(a["indptrA"], a["indicesA"], a["dataA"], ec_keep)
    assert f["kept_cells"].tolist() == kept and 0 < len(kept) <= n_cells
    if mincount > 0:
        assert len(kept) < n_cells
    for k, exp in (("indptrA", a_ptr), ("indicesA", a_idx), ("dataA", a_dat), ("indptrN", n_ptr), ("indicesN", n_idx), ("dataN", n_dat)):
        assert np.array_equal(f[k], exp), k


def test_multisample_over_shards_equals_one_handle():
    """Multisample across GPUs, device side on one card: three contiguous read shards (every cell has reads in all of them),
    ECs merged by key range and adopted by a multisample root, the root's EC keys looked up by every shard
    (ecb_ms_local_triples_device), the shards' triples combined on the root (ecb_ms_adopt_triples_device)
    == export_pairs of one handle over the whole stream."""
    import torch
    from alntools_amd import dist as ecdist
    spec = synth.SynthSpec(60000, 3000, 8, paired=True)
    dev = torch.device("cuda:0")
    whole = synth.generate(spec, 0, spec.n_reads, device=dev)
    n_reads = whole["n_reads"]
    g = np.arange(n_reads, dtype=np.uint64)
    meta = (((g * np.uint64(2654435761)) % np.uint64(211)) | ((g % np.uint64(3)) << np.uint64(22))).astype(np.uint32)
    with ecb.EcBuilder(spec.n_loci, spec.n_haps, multisample=True) as one:
        one.push_device(whole["read_id"], whole["locus"], whole["hapflag"])
        one.push_cells(meta, 0)
        s1 = one.finalize()
        exp = one.export_pairs()
        exp_a = one.export()
    cuts = [0, 17000, 25000, spec.n_reads]
    P = 3
    shards, pieces, sizes, base = [], [], [], 0
    for a, b_ in zip(cuts[:-1], cuts[1:]):
        t = synth.generate(spec, a, b_, device=dev)
        b = ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12, multisample=True)
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        b.push_cells(meta[base:base + t["n_reads"]], 0)
        eng = ecdist.GpuEngine(b, dev)
        nreads = b.table_sizes()[2]
        pieces.append(eng.table_export_parts(base, P))
        sizes.append((nreads,) + b.counters()[:2])
        shards.append((eng, base))
        base += nreads
    assert base == n_reads
    root = ecdist.GpuEngine(ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12, multisample=True), dev)
    adopted = []
    for q in range(P):
        part = ecdist.GpuEngine(ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12), dev)
        part.table_merge_many([(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                               for ent, prs, eoff, poff in pieces if eoff[q + 1] > eoff[q]])
        pe_n, pp_n, _ = part.table_sizes()
        adopted.append(part.table_export(0) + (pe_n, pp_n))
        part.b.close()
    root.table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
    root.add_counters(sum(s[1] for s in sizes), sum(s[2] for s in sizes), base)
    s = root.b.finalize()
    assert s["n_ecs"] == s1["n_ecs"] and s["nnz_n"] == 0
    with pytest.raises(ecb.EcbError):
        root.b.export_pairs()                                            # no triples adopted yet
    keys, nnz = root.ec_keys(s["n_ecs"])
    assert nnz == s["nnz_a"]
    tables = []
    for eng, b0 in shards:
        key, cnt, first, n = eng.ms_local_triples(keys, s["n_ecs"], nnz, b0)
        sk = (key[:n] & ~0xFFFFFFFF) | ((key[:n] & 0x3FFFFF) << 10) | ((key[:n] >> 22) & 0x3FF)    # sorted by (EC, cell, file)
        assert n > 0 and bool((sk[1:] > sk[:-1]).all())
        tables.append((key, cnt, first, n))
    nt = root.ms_adopt_triples(tables)
    assert nt == s1["nnz_n"] and nt < sum(t[3] for t in tables)          # cells straddle the shards: triples were combined
    got = root.b.export_pairs()
    for k in ("ec", "cell", "file", "count", "first"):
        assert np.array_equal(got[k], exp[k]), k
    got_a = root.b.export()
    for k in ("indptrA", "indicesA", "dataA"):
        assert np.array_equal(got_a[k], exp_a[k]), k
    for eng, _ in shards:
        eng.b.close()
    root.b.close()


def test_multi_gpu_entry_points_refuse_wrong_states():
    """State machine of the table / multisample exchange calls: loud errors, never a silent wrong result."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    spec = synth.SynthSpec(2000, 300, 4, paired=False)
    t = synth.generate(spec, 0, spec.n_reads, device=dev)
    b = ecb.EcBuilder(spec.n_loci, spec.n_haps)                          # not multisample
    b.push_device(t["read_id"], t["locus"], t["hapflag"])
    eng = ecdist.GpuEngine(b, dev)
    ne, npairs, nreads = b.table_sizes()
    ent = torch.empty(ne * 4, dtype=torch.int64, device=dev)
    prs = torch.empty(npairs, dtype=torch.int64, device=dev)
    with pytest.raises(ecb.EcbError):
        b.table_export_parts_device(ent, prs, 0, 0)                      # 1 .. 64 parts
    with pytest.raises(ecb.EcbError):
        b.table_export_parts_device(ent, prs, 0, 65)
    with pytest.raises(ecb.EcbError):
        b.table_export_parts_device(ent, prs, (1 << 32) - 10, 2)         # read numbering beyond 2^32
    eo, po = b.table_export_parts_device(ent, prs, 0, 64)                # the most parts: everything accounted for
    assert eo[-1] == ne and po[-1] <= npairs and len(eo) == 65
    with pytest.raises(ecb.EcbError):
        t2 = synth.generate(spec, 0, 10, device=dev)
        b.push_device(t2["read_id"], t2["locus"], t2["hapflag"])         # the table was exported: the stream is closed
    keys = torch.zeros(2, dtype=torch.int64, device=dev)
    csr = (torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
           torch.ones(1, dtype=torch.int32, device=dev))
    out = (torch.empty(nreads, dtype=torch.int64, device=dev), torch.empty(nreads, dtype=torch.int32, device=dev),
           torch.empty(nreads, dtype=torch.int32, device=dev))
    with pytest.raises(ecb.EcbError):
        b.ms_local_triples_device(keys, *csr, 1, 0, *out)                # handle without ECB_F_MULTISAMPLE
    with pytest.raises(ecb.EcbError):
        b.export_ec_keys_device(keys)                                    # before finalize
    with pytest.raises(ecb.EcbError):
        b.ms_adopt_triples_device([out + (0,)])
    ms = ecb.EcBuilder(spec.n_loci, spec.n_haps, multisample=True)
    ms.push_device(t["read_id"], t["locus"], t["hapflag"])
    with pytest.raises(ecb.EcbError):
        ms.ms_local_triples_device(keys, *csr, 1, 0, *out)               # cells were never pushed
    ms.push_cells(np.zeros(nreads, np.uint32), 0)
    with pytest.raises(ecb.EcbError):
        ms.ms_local_triples_device(keys, *csr, 1, 0, *out)               # its ECs are not in that key list
    with pytest.raises(ecb.EcbError):
        ms.ms_adopt_triples_device([out + (0,)])                         # not an adopting, finalized handle
    b.close()
    ms.close()


def test_tuples_pushed_as_whole_tiles_equal_tuples_pushed_as_three_arrays():
    """``ecb_push_device_tiled``: one buffer of tiles -- 512 read ids | 512 loci | 512 haplotype/flag words per tile -- instead of three arrays.
    Same result as the oracle's on: a stream that ends inside a tile, one shorter than a tile, reads longer than a tile (the long-read path
    indexes the tiles too), a stream pushed half as tiles and half as arrays, the short-read and the paralog compilations, a table that has to
    grow; the exactness pass reads the tiles; the entry point refuses what it cannot take."""
    import torch
    from oracle import c_oracle
    dev = torch.device("cuda:0")

    def up(t):
        return [torch.from_numpy(t[k].view(np.int32)).to(dev) for k in ("read_id", "locus", "hapflag")]

    cases = []
    for spec in (synth.SynthSpec(30011, 3000, 8, paired=True), synth.SynthSpec(7, 50, 2, paired=False),
                 synth.SynthSpec(90000, 2000, 2, paired=False, n_variants=2), synth.SynthSpec(60000, 9000, 8, paired=True, paralog_pct=60)):
        t = synth.generate(spec, 0, spec.n_reads)
        cases.append((t, spec.n_loci, spec.n_haps))
    T, H = 5000, 4
    big = [(1, (i * 7) % T, i % H, 0) for i in range(6000)]
    recs = [(0, 5, 1, 0), (0, 5, 2, 0)] + big + [(2, 5, 2, 0)] + [(3, l, h, f) for (_, l, h, f) in reversed(big)] + [(4, 4999, 3, 0)]
    cases.append((_hand(recs, H), T, H))
    for t, n_loci, n_haps in cases:
        exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], n_haps, threads=4)
        d = up(t)
        n = len(t["read_id"])
        tiles = ecb.tile_tuples(*d)
        assert tiles.numel() == (n + 511) // 512 * 1536
        for hint, cap in ((0, 1 << 16), (exp["n_reads"], 1 << 10)):
            with ecb.EcBuilder(n_loci, n_haps, ec_capacity=cap) as b:
                b.hint_reads(hint)
                b.push_device_tiled(tiles, n)
                s = b.finalize()
                _check(b.export(), s, exp)
                b.reset()
                b.push_device_tiled(tiles, n)
                assert b.verify_device_tiled(tiles, n)[0] == 0          # (second figure: reads that took the long-read compare)
                assert b.verify_device(*d) == b.verify_device_tiled(tiles, n)      # (the same records as three arrays)
        # first part as tiles, the rest as three arrays (cut at a tile boundary where a read starts)
        rid = t["read_id"]
        cut = (n // 2) & ~511
        while 0 < cut < n and rid[cut] == rid[cut - 1]:
            cut += 512
        if 0 < cut < n:
            with ecb.EcBuilder(n_loci, n_haps) as b:
                b.push_device_tiled(tiles[:cut // 512 * 1536], cut)
                b.push_device(*[x[cut:] for x in d])
                s = b.finalize()
                _check(b.export(), s, exp)
    with ecb.EcBuilder(10, 2, track_ranges=True) as b:          # the range update wants its fourth stream
        with pytest.raises(ecb.EcbError) as e:
            b.push_device_tiled(torch.zeros(1536, dtype=torch.int32, device=dev), 5)
        assert e.value.code == -6
    with ecb.EcBuilder(10, 2) as b:
        with pytest.raises(ValueError):
            b.push_device_tiled(torch.zeros(1536, dtype=torch.int32, device=dev), 600)      # two tiles' worth of records, one tile of buffer


def test_counts_survive_a_second_finalize_and_a_table_export_after_the_first():
    """What finalize leaves in the table -- every EC's reads, first read and key -- is what a second finalize and a table export
    after the first read again: both must give what the first gave.  Reference: N = reads per EC, ``bam_utils.py:309-312``."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    spec = synth.SynthSpec(n_reads=60000, n_loci=3000, n_haps=8, paired=True)
    t = synth.generate(spec, 0, spec.n_reads, device=dev)
    exp = _expect(synth.generate(spec, 0, spec.n_reads), spec.n_loci, spec.n_haps)
    with ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12) as b, ecb.EcBuilder(spec.n_loci, spec.n_haps, ec_capacity=1 << 12) as plain:
        b.push_device(t["read_id"], t["locus"], t["hapflag"])
        plain.push_device(t["read_id"], t["locus"], t["hapflag"])
        s1 = b.finalize()
        first = b.export()
        _check(first, s1, exp)
        s2 = b.finalize()                                        # again: everything is derived from the table once more
        again = b.export()
        assert s1 == s2
        for k in first:
            assert np.array_equal(first[k], again[k]), k
        # the table of the finalized handle, exported: the same entries (hash, reads, first read, key length) as a handle that was never finalized
        ent, _ = ecdist.GpuEngine(b, dev).table_export(0)
        ent0, _ = ecdist.GpuEngine(plain, dev).table_export(0)
        ne = b.table_sizes()[0]
        assert ne == plain.table_sizes()[0] == s1["n_ecs"]
        e, e0 = ent[:ne * 4].view(-1, 4).cpu().numpy(), ent0[:ne * 4].view(-1, 4).cpu().numpy()
        e, e0 = e[np.argsort(e[:, 0], kind="stable")], e0[np.argsort(e0[:, 0], kind="stable")]
        assert np.array_equal(e[:, 0], e0[:, 0]) and np.array_equal(e[:, 2], e0[:, 2]) and np.array_equal(e[:, 3] >> 32, e0[:, 3] >> 32)
        assert int((e[:, 2] & 0xFFFFFFFF).sum()) == s1["n_reads"]


@pytest.mark.parametrize("ec_capacity", [1 << 10, 1 << 14, 1 << 21])
def test_rows_of_every_length_leave_in_column_order(ec_capacity):
    """ECs of 1 .. 24 loci side by side, loci in descending order in the stream: rows short enough for the slot's own pairs, rows that
    continue in the key arena, and rows of more than sixteen (one wave each) meet in the same waves of the CSR emit, and every one of
    them must leave with its columns ascending (scipy's csc -> csr, ``bin_utils.py:211``).  The table sizes put the counting
    partition at one range, at a few, and at 512 (ensure_counts); first reads sit on both sides of every 512-read boundary of the
    first-appearance bitmap."""
    T, H = 200000, 8
    rng = np.random.default_rng(1234)
    n_ecs = 3000
    recs = []
    rid = 0
    for k in range(n_ecs):
        n = k % 24 + 1
        base = (k * 37) % (T - 64 * 24)
        loci = (base + np.arange(n) * (1 + k % 5))[::-1]
        haps = rng.integers(0, H, size=n)
        recs += [(rid, int(l), int(h), 0) for l, h in zip(loci, haps)]
        if n > 3:
            recs.append((rid, int(loci[0]), int(haps[0]), 0))                    # a duplicate (read, target): collapses
        rid += 1
    first_lap = list(recs)
    for (r, l, h, f) in first_lap[: len(first_lap) // 2]:        # the first half of the ECs once more, as new reads
        recs.append((rid + r, l, h, f))
    t = _hand(recs, H)
    out, sizes = _run_host(t, T, H, ec_capacity=ec_capacity)
    exp = _expect(t, T, H)
    _check(out, sizes, exp)
    assert sizes["n_ecs"] == len(exp["count"]) and int(out["dataN"].max()) == 2
    rows = np.diff(out["indptrA"])
    assert rows.max() == 24 and rows.min() == 1
    for a, b in zip(out["indptrA"][:-1], out["indptrA"][1:]):
        assert np.all(np.diff(out["indicesA"][a:b]) > 0)


def test_long_keys_through_export_merge_and_adopt():
    """Reads of 3, 30, 300 and 900 loci (keys that fit the slot, continue in the arena, take a wave of their own when exported, and
    the long-read path of the stream kernel) in two shards that share some of their ECs: every shard cut into key ranges, the ranges
    merged and adopted by a root as the multi-GPU protocol does (``alntools_amd/dist.py``; the reference's ordered merge,
    ``bam_utils.py:680-724``) == one handle over both shards == the oracle."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    T, H, P = 60000, 8, 3
    rng = np.random.default_rng(77)

    def shard(seed_bases, first_rid):
        recs, rid = [], first_rid
        for k, base in enumerate(seed_bases):
            n = (3, 30, 300, 900)[k % 4]
            loci = base + np.arange(n) * 2
            haps = rng.integers(0, H, size=n)
            order = rng.permutation(n)
            recs += [(rid, int(loci[j]), int(haps[j]), 0) for j in order]
            recs += [(rid, int(loci[0]), int((haps[0] + 1) % H), 0)]              # one locus with two haplotypes
            rid += 1
        return recs
    bases_a = [int(b) for b in rng.integers(0, T - 2000, size=40)]
    bases_b = bases_a[:12] + [int(b) for b in rng.integers(0, T - 2000, size=28)]        # twelve ECs... of the same loci -- but the haplotypes are drawn anew: mostly new ECs, same loci
    ra, rb = shard(bases_a, 0), shard(bases_b, 0)
    both = _hand(ra + [(r + 40, l, h, f) for (r, l, h, f) in rb] + [(80 + r, l, h, f) for (r, l, h, f) in ra[:len(ra) // 2]], H)     # + the first shard's first half again: shared ECs for certain
    shards = [_hand(ra, H), _hand(rb + [(40 + r, l, h, f) for (r, l, h, f) in ra[:len(ra) // 2]], H)]
    exp = _expect(both, T, H)
    pieces, sizes, base = [], [], 0
    for t in shards:
        b = ecb.EcBuilder(T, H, ec_capacity=1 << 10)
        b.push(t["read_id"], t["locus"], t["hapflag"])
        eng = ecdist.GpuEngine(b, dev)
        nreads = b.table_sizes()[2]
        pieces.append(eng.table_export_parts(base, P))
        sizes.append((nreads,) + b.counters()[:2])
        base += nreads
        b.close()
    root = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 10), dev)
    for q in range(P):
        part = ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 10), dev)
        tabs = [(ent[eoff[q] * 4:eoff[q + 1] * 4], eoff[q + 1] - eoff[q], prs[poff[q]:poff[q + 1]], poff[q + 1] - poff[q])
                for ent, prs, eoff, poff in pieces if eoff[q + 1] > eoff[q]]
        part.table_merge_many(tabs)
        pe_n, pp_n, _ = part.table_sizes()
        pe, pp = part.table_export(0)
        root.table_adopt(pe, pe_n, pp, pp_n)
        part.b.close()
    root.add_counters(sum(s[1] for s in sizes), sum(s[2] for s in sizes), base)
    s = root.b.finalize()
    _check(root.b.export(), s, exp)
    assert int(np.diff(exp["indptr"]).max()) == 900 and s["n_reads"] == base
    root.b.close()


def test_bench_dump_outputs_are_what_the_timed_steps_computed(tmp_path):
    """``bench.py --workload c1 --dump-outputs DIR`` in a process of its own: the files hold the last timed step's CSR A, counts and
    counters, equal to the oracle's on the same seeded tuples; the result line reports the steps asked for and their time."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--dump-outputs", str(d)], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    spec = synth.SynthSpec(10000, 1000, 2)
    t = synth.generate(spec, 0, spec.n_reads)
    exp = _expect(t, spec.n_loci, spec.n_haps)
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(a.dtype == np.float64 for a in got.values())
    for name, key in (("indptrA", "indptr"), ("indicesA", "indices"), ("dataA", "data"), ("dataN", "count")):
        assert np.array_equal(got[name], np.asarray(exp[key], dtype=np.float64)), name
    n_ecs, nnz_a, n_samples, nnz_n, n_all, n_valid, n_reads = got["sizes"]
    assert (n_ecs, nnz_a, n_all, n_valid, n_reads) == (len(exp["count"]), len(exp["indices"]), exp["n_all"], exp["n_valid"],
                                                       int(np.sum(exp["count"])))


def test_bench_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """``bench.py --workload c1``: a plain run prints the headline and measures nothing besides it (no transposition step, no
    exactness pass, no copy peaks, no host-side legs); ``--full`` adds them after the same timed steps, the exactness pass at 0."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--steps", "2", "--warmup", "1", *extra],
                           cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    plain = run()
    assert plain["unit"] == "alignments/s" and plain["higher_is_better"] is True and plain["dtype"] == "u32"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(plain["config"]["records"] / (plain["ms_per_step"] * 1e-3))
    assert plain["step_emase_ms"] is None and plain["config"]["exactness_pass"] is None
    assert plain["config"]["sensors_under_load"] is None and plain["roofline"]["peak_measured_copy"] is None
    assert not {"cpu_baseline", "parity_vs_oracle", "secondary", "cpu_baseline_py", "h2d_inclusive", "e2e_from_bam"} & set(plain)
    full = run("--full", "--no-cpu-baseline")
    assert full["steps"] == 2 and full["ms_per_step"] > 0 and full["config"]["records"] == plain["config"]["records"]
    assert full["config"]["ecs"] == plain["config"]["ecs"] and full["config"]["nnz_a"] == plain["config"]["nnz_a"]
    assert full["step_emase_ms"] > 0
    assert full["config"]["exactness_pass"]["reads_differing_from_their_ec_key"] == 0
    assert full["roofline"]["peak_measured_copy"] > 0
