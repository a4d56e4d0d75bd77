"""``ecb_best_strata`` / ``ecb_best_strata_device`` (``--best-strata``) against the rule as ``tests/strata_checker.py`` states it: every
output compared exactly.  The sizes sit on the spans the kernels work in -- L records per lane, W per wave, G per workgroup, pinned to
the source by ``tests/test_strata_constants.py`` -- and are the smallest at which a segmented reduction goes wrong."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_strata as es

import strata_checker as sk
from test_strata_constants import G, L, W

pytestmark = pytest.mark.gpu
PASS, FAIL = 0x0, 0x4
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NONE = 0xFFFFFFFF


def build(reads, first_id=0, lead=0):
    """A stream from ``reads`` = lists of ``(passes, score)`` records, each beginning with a passing record (where the id steps); the
    first read's id is ``first_id``; ``lead`` non-passing records, carrying ``first_id - 1``, open the stream."""
    rid, hf, sc = [(first_id - 1) % (1 << 32)] * lead, [FAIL] * lead, [I32_MIN] * lead
    for k, read in enumerate(reads):
        assert read[0][0]
        for ok, s in read:
            rid.append((first_id + k) % (1 << 32))
            hf.append(PASS if ok else FAIL)
            sc.append(s)
    return np.array(rid, dtype=np.uint32), np.array(hf, dtype=np.uint32), np.array(sc, dtype=np.int32)


def agree(rid, hf, sc, lowest=True, **kw):
    want = sk.best_strata(rid, hf, sc, lowest)
    got = es.best_strata(rid, hf, sc, lowest=lowest, **kw)
    assert sk.breach(rid, hf) is None
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    assert len(bad) == 0, "record %d of %d: id %#x flags %#x, want %#x %#x" % (bad[0], len(rid), got[0][bad[0]], got[1][bad[0]], want[0][bad[0]], want[1][bad[0]])
    assert got[2] == want[2]
    return got


def short_reads(rng, n, heads=(), p_head=0.3, p_fail=0.2, n_scores=3, first_id=0):
    """``n`` records of short reads with scores 0 .. n_scores - 1; a read starts at every index of ``heads``."""
    head = rng.random(n) < p_head
    head[list(heads)] = True
    head[0] = True
    ok = (rng.random(n) >= p_fail) | head
    rid = (np.cumsum(head) - 1 + first_id).astype(np.uint32)
    return rid, np.where(ok, PASS, FAIL).astype(np.uint32), rng.integers(0, n_scores, size=n).astype(np.int32)


@pytest.mark.parametrize("lowest", [True, False], ids=["lowest", "highest"])
def test_tiny_streams(lowest):
    rng = np.random.default_rng(1)
    for n in (1, L - 1, L, L + 1):
        for _ in range(6):
            agree(*short_reads(rng, n, p_head=0.5), lowest=lowest)


def test_short_reads_at_every_offset():
    rng = np.random.default_rng(2)
    for length in range(1, L + 2):
        for offset in range(L):
            for _ in range(3):
                read = [(True, int(rng.integers(0, 3)))] + [(bool(rng.random() < 0.8), int(rng.integers(0, 3))) for _ in range(length - 1)]
                before = [(True, 1)] * offset
                reads = ([before] if offset else []) + [read, [(True, 0), (True, 2)]]
                agree(*build(reads))
                agree(*build(reads), lowest=False)


@pytest.mark.parametrize("n", [3 * G, 3 * G - 1, 2 * G + W + 5])
def test_a_read_boundary_around_every_span(n):
    rng = np.random.default_rng(3)
    edges = [b + d for b in (W, G, 2 * G, n - 1) for d in (-1, 0, 1) if 0 < b + d < n]
    for b in edges:
        # short reads all round, then the same boundary between two reads that fill the records before and behind it
        agree(*short_reads(rng, n, heads=[b]))
        rid, hf, sc = short_reads(rng, n, heads=[b])
        lo, hi = max(b - W - 3, 0), min(b + W + 3, n)
        rid[lo:b] = rid[lo]
        rid[b:hi] = rid[lo] + 1
        rid[hi:] = rid[hi:] - rid[hi] + rid[lo] + 2 if hi < n else rid[hi:]
        hf[b] = PASS
        if hi < n:
            hf[hi] = PASS
        agree(rid, hf, sc, lowest=bool(b % 2))


def _patterns(n):
    mid = n // 2
    one = lambda at: [0 if i in at else 1 for i in range(n)]
    return {"first": one({0}), "last": one({n - 1}), "middle": one({mid}), "both-ends": one({0, n - 1}), "all-tied": [7] * n,
            "rising": list(range(n)), "falling": list(range(n, 0, -1))}


@pytest.mark.parametrize("length", [3 * G + 1, 2 * W + 1], ids=["3G+1", "2W+1"])
@pytest.mark.parametrize("lowest", [True, False], ids=["lowest", "highest"])
def test_long_reads(length, lowest):
    rng = np.random.default_rng(4)
    for name, scores in _patterns(length).items():
        if not lowest:
            scores = [-s for s in scores]
        for offset in (0, 3, W - 2):
            long_read = [(True, s) for s in scores]
            if name == "middle":                        # (a non-passing record inside does not matter, whatever its score)
                long_read[length // 3] = (False, I32_MIN if lowest else I32_MAX)
            before = [[(True, int(rng.integers(0, 3)))] for _ in range(offset)]
            agree(*build(before + [long_read, [(True, 1), (True, 0)], [(True, 0)]]), lowest=lowest)


def test_the_first_passing_record_dropped():
    worked = (np.array([NONE, 0, 0, 0, 0, 0, 1], dtype=np.uint32), np.array([FAIL, PASS, FAIL, PASS, PASS, PASS, PASS], dtype=np.uint32),
              np.array([99, 2, -5, 1, 1, 3, 0], dtype=np.int32))
    got = agree(*worked)
    assert got[0].tolist() == [NONE, NONE, NONE, 0, 0, 0, 1] and got[1].tolist() == [FAIL, PASS | 0x4004, FAIL, PASS, PASS, PASS | 0x4004, PASS]
    assert got[2] == (5, 3, 2, 1)
    read = [(True, 2), (False, 0), (True, 1), (False, 0), (True, 0), (True, 5)]
    for first_id, lead in ((0, 0), (0, 3), (1, 0), (5, 2), ((1 << 32) - 3, 0), ((1 << 32) - 3, 4)):
        # alone; behind a read whose non-passing tail lies before it; and twice in a row
        agree(*build([read], first_id, lead))
        agree(*build([[(True, 0), (False, 9)], read, read, [(True, 1)]], first_id, lead))
    # a stream that opens with the previous read's non-passing tail, then that id's own passing records (no step): still one read
    rid = np.array([4, 4, 4, 4, 5, 5], dtype=np.uint32)
    agree(rid, np.array([FAIL, FAIL, PASS, PASS, PASS, PASS], dtype=np.uint32), np.array([0, 0, 3, 2, 1, 0], dtype=np.int32))
    # ... across a wave's and a workgroup's span: the dropped records of the first W + 2 (G + 2) carry the read before
    for span in (W, G):
        read = [(True, 3)] + [(bool(i % 3), 2) for i in range(span)] + [(True, 1), (True, 1), (True, 2)]
        agree(*build([[(True, 0)], read, [(True, 0)]], first_id=0))
        agree(*build([read], first_id=0))


@pytest.mark.parametrize("lowest", [True, False], ids=["lowest", "highest"])
def test_extreme_scores(lowest):
    vals = [I32_MIN, -1, 0, I32_MAX]
    reads = [[(True, a), (True, b)] for a in vals for b in vals] + [[(True, v) for v in vals], [(True, v) for v in reversed(vals)]]
    agree(*build(reads), lowest=lowest)


def test_each_term_of_the_filter_with_garbage_scores_on_the_rejected():
    rejected = [0x4, 0x1, 0x1 | 0x2 | 0x80, 0x1 | 0x2 | 0x1000, 0x1 | 0x2 | 0x2000, 0x1 | 0x80, 0x3 | 0x4]
    passing = [0x0, 0x1 | 0x2, 0x1000, 0x2000, 0x80, 0x1 | 0x2 | 0x40, 0x10 | (3 << 16), 0x8000]
    for hf in rejected:
        assert not sk.passes(hf)
    for hf in passing:
        assert sk.passes(hf)
    for lowest in (True, False):
        garbage = I32_MIN if lowest else I32_MAX
        rid, hfs, sc = [], [], []
        for r, bad in enumerate(rejected):
            for k, good in enumerate(passing):
                rid += [r * len(passing) + k] * 4
                hfs += [good, bad, good, bad]
                sc += [1, garbage, 1 if k % 2 else 0, garbage]
        got = agree(np.array(rid, dtype=np.uint32), np.array(hfs, dtype=np.uint32), np.array(sc, dtype=np.int32), lowest=lowest)
        assert got[2][0] == 2 * len(rid) // 4


def zipf_stream(seed, n=200000):
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.zipf(1.6, size=n), 5 * G)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    head = np.zeros(int(lens.sum()), dtype=bool)
    head[np.cumsum(lens) - lens] = True
    head = head[:n]
    ok = (rng.random(n) >= 0.15) | head
    return ((np.cumsum(head) - 1).astype(np.uint32), np.where(ok, PASS, FAIL).astype(np.uint32) | (rng.integers(0, 2, size=n) << 16).astype(np.uint32),
            rng.integers(0, 4, size=n).astype(np.int32))


_ZIPF = {}


def _zipf(lowest):
    if lowest not in _ZIPF:
        s = zipf_stream(11)
        _ZIPF[lowest] = (s, sk.best_strata(*s, lowest=lowest))
    return _ZIPF[lowest]


@pytest.mark.parametrize("lowest", [True, False], ids=["lowest", "highest"])
def test_a_random_stream_with_zipf_read_lengths(lowest):
    s, want = _zipf(lowest)
    got = es.best_strata(*s, lowest=lowest)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert want[2][2] > 10000 and want[2][3] > 1000 and np.bincount(s[0]).max() > G


def test_the_output_is_a_stream_the_handle_takes():
    import torch
    s, want = _zipf(True)
    rng = np.random.default_rng(5)
    n_loci = 50
    locus = rng.integers(0, n_loci, size=len(s[0])).astype(np.uint32)
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in (s[0], s[1], s[2], locus)]
    out_id, out_hf, counts = es.best_strata(dev[0], dev[1], dev[2])
    assert counts == want[2]
    with ecb.EcBuilder(n_loci, 2) as b:
        b.push_device(out_id, dev[3], out_hf)
        sizes = b.finalize()
        got = b.export()
    keep = sk.kept_mask(*s)
    assert keep.sum() == len(keep) - want[2][2]
    with ecb.EcBuilder(n_loci, 2) as b:
        b.push(want[0][keep], locus[keep], want[1][keep])
        ref_sizes = b.finalize()
        ref = b.export()
    assert sizes["valid_alignments"] == ref_sizes["valid_alignments"] == want[2][1] and sizes["n_reads"] == ref_sizes["n_reads"]
    assert sizes["all_alignments"] == len(keep) and sizes["n_ecs"] == ref_sizes["n_ecs"]
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_in_place_twice_tensors_and_poisoned_scratch_give_the_same_bytes(monkeypatch):
    import torch
    s, want = _zipf(False)
    first = es.best_strata(*s, lowest=False)
    again = es.best_strata(*s, lowest=False)
    rid, hf = s[0].copy(), s[1].copy()
    inpl = es.best_strata(rid, hf, s[2], lowest=False, inplace=True)
    assert inpl[0] is rid and inpl[1] is hf
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in s]
    tens = es.best_strata(*dev, lowest=False)
    tens_in = es.best_strata(dev[0], dev[1], dev[2], lowest=False, inplace=True)
    assert tens_in[0] is dev[0] and tens_in[1] is dev[1]
    monkeypatch.setenv("ECB_POISON_SCRATCH", "1")
    poisoned = [es.best_strata(*s, lowest=False) for _ in range(2)]
    monkeypatch.delenv("ECB_POISON_SCRATCH")
    for got in [first, again, inpl] + poisoned:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    for got in (tens, tens_in):
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0]) and np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1])
        assert got[2] == want[2]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw(rid, hf, sc, n=None, mode=0, out_id=None, out_hf=None, counts=True):
    lib = es.load()
    n = len(rid) if n is None else n
    oi = np.full(len(rid), 0x5C5C5C5C, dtype=np.uint32) if out_id is None else out_id
    oh = np.full(len(rid), 0x5C5C5C5C, dtype=np.uint32) if out_hf is None else out_hf
    cnt = (C.c_uint64 * 4)(*[7] * 4)
    P = ecb._ptr
    rc = lib.ecb_best_strata(0, P(rid), P(hf), P(sc), n, mode, P(oi), P(oh), cnt if counts else None)
    return rc, (lib.ecb_last_error(None) or b"").decode(), oi, oh, tuple(cnt)


def test_refused_arguments_write_nothing():
    rid, hf, sc = build([[(True, 1), (True, 0)], [(True, 0)]])
    untouched = lambda r: (r[2] == 0x5C5C5C5C).all() and (r[3] == 0x5C5C5C5C).all() and r[4] == (7,) * 4
    for kw in (dict(n=0), dict(mode=2), dict(mode=0xFFFFFFFF), dict(counts=False)):
        r = _raw(rid, hf, sc, **kw)
        assert r[0] == -1 and r[1].startswith("strata: ") and untouched(r), (kw, r[:2])
    lib = es.load()
    P = ecb._ptr
    cnt = (C.c_uint64 * 4)()
    o1, o2 = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    for args in ((None, P(hf), P(sc), P(o1), P(o2)), (P(rid), None, P(sc), P(o1), P(o2)), (P(rid), P(hf), None, P(o1), P(o2)),
                 (P(rid), P(hf), P(sc), None, P(o2)), (P(rid), P(hf), P(sc), P(o1), None)):
        assert lib.ecb_best_strata(0, args[0], args[1], args[2], 3, 0, args[3], args[4], cnt) == -1
    # an output may be exactly its input; any other overlap is refused
    big = np.zeros(16, dtype=np.uint32)
    big[:3], big[8:11] = rid, hf
    for oi, oh in ((big[1:4], o2), (o1, big[9:12]), (big[8:11], o2), (o1, big[0:3]), (o1, o1), (o1[:], o1), (sc.view(np.uint32), o2)):
        before = big.copy()
        rc = lib.ecb_best_strata(0, P(big[0:3]), P(big[8:11]), P(sc), 3, 0, P(oi), P(oh), cnt)
        assert rc == -1 and b"overlaps" in lib.ecb_last_error(None) and np.array_equal(big, before)
    assert lib.ecb_best_strata(0, P(big[0:3]), P(big[8:11]), P(sc), 3, 0, P(big[0:3]), P(big[8:11]), cnt) == 0
    assert big[:3].tolist() == [NONE, 0, 1] and big[8:11].tolist() == [0x4004, 0, 0] and tuple(cnt) == (3, 2, 1, 1)


@pytest.mark.parametrize("at", [1, L, W - 1, W, G, 2 * G + 1, 2 * G + W + 3])
def test_a_broken_contract_names_the_lowest_offender_and_writes_nothing(at):
    rng = np.random.default_rng(at)
    n = 2 * G + W + 5
    for reason in ("falls", "steps by more than 1", "steps on a record that does not pass the filter"):
        rid, hf, sc = short_reads(rng, n)
        if reason == "falls":
            rid[at:] -= np.uint32(rid[at] - rid[at - 1] + 1)
        elif reason == "steps by more than 1":
            rid[at:] += np.uint32(2)
        else:
            rid[at:] += np.uint32(1 - (rid[at] - rid[at - 1]))
            hf[at] = FAIL
        if at + 300 < n:                                  # a second, higher offender: the lowest is named
            rid[at + 300:] += np.uint32(5)
        assert sk.breach(rid, hf) == (at, "read_id " + reason)
        rc, msg, oi, oh, cnt = _raw(rid, hf, sc)
        assert rc == ecb.ECB_ERR_CONTRACT and msg == "strata: record %d: read_id %s" % (at, reason), msg
        assert (oi == 0x5C5C5C5C).all() and (oh == 0x5C5C5C5C).all() and cnt == (7,) * 4
        with pytest.raises(es.StrataContractError) as e:
            es.best_strata(rid, hf, sc)
        assert e.value.record == at
    # ids that make no sense at all address nothing outside the buffers: the call is refused, and the next one is right
    rid = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    rc, msg, oi, oh, cnt = _raw(rid, hf, sc)
    assert rc == ecb.ECB_ERR_CONTRACT and (oi == 0x5C5C5C5C).all() and (oh == 0x5C5C5C5C).all()
    agree(*short_reads(rng, n))


# ---- end to end through the command line --------------------------------------------------------------------------------------------------
def _g4b_gen():
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import g4b_gen
    return g4b_gen


def _tagged_files(seed, n_files=3, reads=260):
    """Seeded records in the manner of ``tests/golden/g4b_gen.py`` (its references and read names; names without a space: with the
    reference's untrimmed-name quirk every record of a spaced name is a run of its own), each with seeded NM, AS and -- four times
    in five -- YS tags.  -> [(records, tags, {TAG: scores})] per file."""
    g4b_gen = _g4b_gen()
    rng = np.random.RandomState(seed)
    out = []
    for fi in range(n_files):
        recs, tags, nm_s, as_s = [], [], [], []
        for r in range(reads):
            name = g4b_gen._qname("f%dr%05d" % (fi, r), "BC%04d" % rng.randint(5))
            if rng.rand() < 0.05:
                recs.append((name, 4, -1, -1, -1, -1))
                tags.append([("YS", "i", 0)] if rng.rand() < 0.5 else [])          # (not passing: its tags are never asked for)
                nm_s.append(0); as_s.append(0)
                continue
            g = int(rng.randint(g4b_gen.N_GENES))
            tids = [2 * g, 2 * g + 1] if rng.rand() < 0.8 else [2 * g + int(rng.randint(2))]
            if rng.rand() < 0.3:
                g2 = (g + 1 + int(rng.randint(3))) % g4b_gen.N_GENES
                tids += [2 * g2, 2 * g2 + 1]
            for t in tids:
                nm = int(rng.randint(3))
                a = -6 * nm - int(rng.randint(2))
                t_ = [("NM", "C", nm), ("XS", "Z", "x"), ("AS", "c" if rng.rand() < 0.5 else "i", a)]
                ys = None
                if rng.rand() < 0.8:
                    ys = -int(rng.randint(4))
                    t_.append(("YS", "i", ys))
                recs.append((name, 16 if rng.rand() < 0.5 else 0, int(t), int(rng.randint(500)), -1, -1))
                tags.append(t_)
                nm_s.append(nm); as_s.append(a + (ys or 0))
        out.append((recs, tags, {"NM": nm_s, "AS+YS": as_s}))
    return out


def _kept_records(recs, tags, scores, lowest):
    """The records the checker keeps (the non-passing ones stay), on the stream as the tool numbers it: a read is a run of equal names
    among the passing records."""
    rid, cur, last = [], -1, None
    for name, flag, *_ in recs:
        if sk.passes(flag) and name != last:
            cur, last = cur + 1, name
        rid.append(cur % (1 << 32))
    hf = np.array([r[1] for r in recs], dtype=np.uint32)
    keep = sk.kept_mask(np.array(rid, dtype=np.uint32), hf, np.array(scores, dtype=np.int32), lowest)
    assert 0 < keep.sum() < len(keep)
    return [r for r, k in zip(recs, keep) if k], [t for t, k in zip(tags, keep) if k]


_E2E = {}


@pytest.mark.parametrize("decoder", ["py", "c"])
@pytest.mark.parametrize("tag", ["NM", "AS+YS"])
@pytest.mark.parametrize("command", ["bam2ec", "bam2ec-multisample", "bam2emase"])
def test_the_option_end_to_end(tmp_path, monkeypatch, command, tag, decoder):
    """The BAM with all records, run WITH the option, gives the bytes -- ``.bin`` and range file -- of the BAM that holds only the
    checker's kept records, run without it; run without the option it does not."""
    import os
    from click.testing import CliRunner
    from alntools_amd import bamio, cli
    monkeypatch.setenv("ALNTOOLS_DECODER", decoder)
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    if "files" not in _E2E:
        _E2E["files"] = _tagged_files(31)
    files = _E2E["files"]
    multi = command.endswith("multisample")
    refs = _g4b_gen().references()
    for kind in ("all", "kept"):
        os.makedirs(str(tmp_path / kind))
        for fi, (recs, tags, scores) in enumerate(files if multi else files[:1]):
            if kind == "kept":
                recs, tags = _kept_records(recs, tags, scores[tag], lowest=tag == "NM")
            bamio.write_bam(str(tmp_path / kind / ("m_%d.bam" % fi)), refs, recs, tags=tags)

    def run(kind, option):
        out, rng_file = str(tmp_path / ("%s_%d.out" % (kind, option))), str(tmp_path / ("%s_%d.range" % (kind, option)))
        src = str(tmp_path / kind) if multi else str(tmp_path / kind / "m_0.bam")
        args = [command.split("-")[0], src, out, "--rangefile", rng_file] + (["--multisample", "-m", "2"] if multi else []) + \
            (["-s", "S"] if command == "bam2ec" else []) + (["--best-strata", tag] if option else [])
        r = CliRunner().invoke(cli.cli, args)
        assert r.exit_code == 0, (args, r.output, r.exception)
        if command == "bam2emase":
            r = CliRunner().invoke(cli.cli, ["emase2ec", out, out + ".bin"])
            assert r.exit_code == 0, (r.output, r.exception)
            out += ".bin"
        return open(out, "rb").read(), open(rng_file).read()
    with_option, kept_only, without = run("all", 1), run("kept", 0), run("all", 0)
    assert with_option[0] == kept_only[0], "the .bin"
    assert with_option[1] == kept_only[1], "the range file"
    assert without[0] != with_option[0]
