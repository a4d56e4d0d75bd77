"""``--best-strata`` without a GPU: the rule's checker against hand-written records, the score of a record through the writer, the Python
reader and the native decoder (and the decoder's aux walk under sanitizers, as a plain C program), the batch cut, and every refusal of
the command line.  The GPU side is ``tests/test_gpu_best_strata.py``."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bamdec, bamio, ecb_strata as es

import strata_checker as sk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
NONE = 0xFFFFFFFF
P, F, D = 0x0, 0x4, 0x4004            # a passing record, a non-passing one, what a dropped passing record becomes


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------
#        id    flags score | id out  flags out
WORKED = [(NONE, F, 99, NONE, F),
          (0, P, 2, NONE, D),          # read 0's first passing record is dropped: it carries the read before, 0xFFFFFFFF
          (0, F, -7, NONE, F),         # ... and so does the non-passing record behind it
          (0, P, 1, 0, P),             # the first kept record: here the id steps
          (0, P, 1, 0, P),             # a tie is kept
          (0, P, 3, 0, D),             # dropped behind the first kept record: the id stays
          (1, P, 0, 1, P)]
MORE = [(1, F, -100, 1, F),            # a non-passing record's score is never looked at
        (2, P, 5, 2, P),               # a read of one record
        (3, P, -1, 3, P),              # negative scores: -1 is the lowest
        (3, P, 0, 3, D),
        (3, 0x1, -9, 3, 0x1)]          # paired and not properly so: does not pass, whatever its score
HIGHEST = [NONE, NONE, NONE, NONE, NONE, 0, 1, 1, 2, 2, 3, 3], [F, D, F, D, D, P, P, F, P, D, P, 0x1]


def test_the_checker_on_hand_written_records():
    rows = WORKED + MORE
    rid, hf, sc = (np.array([r[k] for r in rows], dtype=dt) for k, dt in ((0, np.uint32), (1, np.uint32), (2, np.int32)))
    assert sk.breach(rid, hf) is None
    out_id, out_hf, counts = sk.best_strata(rid, hf, sc, lowest=True)
    assert out_id.tolist() == [r[3] for r in rows] and out_hf.tolist() == [r[4] for r in rows]
    assert counts == (8, 5, 3, 1)
    assert sk.kept_mask(rid, hf, sc).tolist() == [r[4] != D for r in rows]
    out_id, out_hf, counts = sk.best_strata(rid, hf, sc, lowest=False)
    assert out_id.tolist() == HIGHEST[0] and out_hf.tolist() == HIGHEST[1] and counts == (8, 4, 4, 2)
    # the worked case alone, and the breaches the library names
    w = [np.array([r[k] for r in WORKED]) for k in range(3)]
    assert sk.best_strata(w[0].astype(np.uint32), w[1].astype(np.uint32), w[2].astype(np.int32))[2] == (5, 3, 2, 1)
    assert sk.breach([0, 1, 1, 0], [P] * 4) == (3, "read_id falls")
    assert sk.breach([0, 0, 2], [P] * 3) == (2, "read_id steps by more than 1")
    assert sk.breach([NONE, 0, 1], [F, P, F]) == (2, "read_id steps on a record that does not pass the filter")
    assert sk.breach([NONE - 1, NONE, 0], [F, P, P]) is None


def test_the_filter_is_the_tuple_contracts():
    from alntools_amd import bam_utils, tuples
    flags = np.arange(0, 0x1000, dtype=np.int64)
    for tid, ntid, npos, bits in ((3, 3, 5, 0), (3, 4, 5, 0x1000), (3, 3, -1, 0x2000), (3, 4, -1, 0x3000)):
        n = len(flags)
        want = tuples.record_valid(flags, np.full(n, tid), np.full(n, ntid), np.full(n, npos))
        assert [sk.passes(int(f) | bits) for f in flags] == want.tolist()
        assert bam_utils.strata_passes(flags | bits | (5 << 16) | 0x4000).tolist() == want.tolist()


# ---- the score of a record --------------------------------------------------------------------------------------------------------------
REFS = [("T0_A", 1000), ("T0_B", 1000)]
EVERY_TYPE = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 200), ("Xs", "s", -3000), ("XS", "S", 60000), ("Xi", "i", -100000),
              ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "some text"), ("XH", "H", "1AE301"), ("XB", "B", ("s", [-1, 2, 3])),
              ("Xb", "B", ("C", [])), ("Xd", "B", ("f", [0.5])), ("Xe", "B", ("I", [7, 8]))]


def _name(i):
    f = ["x%d" % k for k in range(15)]
    f[0], f[14] = "r%03d" % (i // 2), "BC%d" % (i % 3)
    return "|||".join(f)


def _scored_records():
    """-> (records, tags per record, {(tag_a, tag_b): (scores, present)})"""
    widths = [("c", -128), ("c", 127), ("C", 255), ("s", -32768), ("S", 65535), ("i", -(1 << 31)), ("i", (1 << 31) - 1), ("I", 0), ("I", 5),
              ("I", (1 << 32) - 1)]
    recs, tags, nm, as_ys = [], [], [], []
    for i, (typ, v) in enumerate(widths):                 # NM in every integer width, every other type before and after it
        recs.append((_name(i), 0, i % 2, 10 + i, -1, -1))
        tags.append(EVERY_TYPE[:i + 2] + [("NM", typ, v)] + EVERY_TYPE[i + 2:])
        nm.append((min(v, (1 << 31) - 1), 1))
        as_ys.append((0, 0))
    k = len(recs)
    for j, t in enumerate(([("AS", "c", -7)], [("YS", "s", -300), ("AS", "C", 20)], [("AS", "i", (1 << 31) - 1), ("YS", "i", 5)],
                           [("YS", "c", 3)], [], [("AS", "i", -(1 << 31)), ("XZ", "Z", ""), ("YS", "i", -1)], [("AS", "S", 9), ("AS", "c", -2)])):
        recs.append((_name(k + j), 16 if j % 2 else 0, j % 2, 50 + j, -1, -1))
        tags.append(list(t))
        nm.append((0, 0))
    as_ys += [(-7, 1), (-280, 1), ((1 << 31) - 1, 1), (3, 0), (0, 0), (-(1 << 31), 1), (-2, 1)]
    as_only = [(0, 0)] * k + [(-7, 1), (20, 1), ((1 << 31) - 1, 1), (0, 0), (0, 0), (-(1 << 31), 1), (-2, 1)]
    recs.append((_name(99), 4, -1, -1, -1, -1))            # an unmapped record with tags of its own
    tags.append([("NM", "C", 1), ("YS", "i", 4)])
    nm.append((1, 1)); as_ys.append((4, 0)); as_only.append((0, 0))
    return recs, tags, {("NM", None): nm, ("AS", "YS"): as_ys, ("AS", None): as_only}


def _write_raw(path, references, raw_records):
    """A BAM file from records given as bytes (``block_size`` included): what ``bamio.write_bam`` writes, record by record."""
    text = ("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in references)).encode()
    w = bamio.BgzfWriter(path)
    hdr = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(references)))
    for n, l in references:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", l)
    w.write(bytes(hdr))
    w.flush_block()
    for r in raw_records:
        w.write(r)
    w.close()


def _py_scores(path, tag_a, tag_b, batch=4):
    rd = bamio.BamReader(path)
    rd.set_score(tag_a, tag_b)
    got = []
    while True:
        q = rd.read_batch(batch)[0]
        if not q:
            break
        s, p = rd.scores()
        assert len(s) == len(p) == len(q)
        got += list(zip(s.tolist(), p.tolist()))
    rd.close()
    return got


def test_tags_round_trip_through_the_writer_and_the_python_reader(tmp_path):
    recs, tags, want = _scored_records()
    path = str(tmp_path / "scored.bam")
    bamio.write_bam(path, REFS, recs, tags=tags)
    assert [r for r in bamio.BamReader(path)] == recs                      # the fields in front of the tags are read as before
    for (a, b), w in want.items():
        assert _py_scores(path, a, b) == w, (a, b)
    # without tags= the bytes are what they were
    assert bamio.pack_record(*recs[0]) == bamio.pack_record(*recs[0], tags=None) == bamio.pack_record(*recs[0], tags=[])
    plain, again = str(tmp_path / "plain.bam"), str(tmp_path / "again.bam")
    bamio.write_bam(plain, REFS, recs)
    bamio.write_bam(again, REFS, recs, tags=[[]] * len(recs))
    assert open(plain, "rb").read() == open(again, "rb").read()
    assert _py_scores(plain, "NM", None) == [(0, 0)] * len(recs)
    # a score tag that is no integer, and a type nobody knows
    for bad in ([("NM", "f", 1.0)], [("NM", "Z", "3")]):
        bamio.write_bam(path, REFS, recs[:1], tags=[bad])
        with pytest.raises(ValueError, match="not an integer"):
            _py_scores(path, "NM", None)
    body = bamio.pack_record(*recs[0])[4:] + b"XXq\x01"
    _write_raw(path, REFS, [struct.pack("<i", len(body)) + body])
    with pytest.raises(ValueError, match="unknown type"):
        _py_scores(path, "NM", None)


def _native_scores(path, tag_a, tag_b, how, batch=4):
    from alntools_amd.tuples import HeaderMaps, TupleEncoder
    rd = bamdec.NativeBamReader(path, threads=2)
    rd.set_score(tag_a, tag_b)
    enc = TupleEncoder(HeaderMaps(rd.references, rd.lengths))
    got = []
    while True:
        d = rd.read_decoded(batch) if how == "decoded" else rd.read_tuples(batch, enc) if how == "tuples" else rd.read_ms(batch)[0]
        if d is None:
            break
        s, p = rd.scores()
        assert len(s) == len(p) == len(d["pos"])
        got += list(zip(s.tolist(), p.tolist()))
    rd.close()
    return got


@pytest.mark.parametrize("how", ["decoded", "tuples", "ms"])
def test_the_native_decoders_scores_are_the_python_readers(tmp_path, how):
    recs, tags, want = _scored_records()
    path = str(tmp_path / "scored.bam")
    bamio.write_bam(path, REFS, recs, tags=tags)
    for (a, b), w in want.items():
        assert _native_scores(path, a, b, how) == _py_scores(path, a, b) == w, (a, b)
    rd = bamdec.NativeBamReader(path)                       # off, as a handle starts: no scores, and none after switching it off again
    assert rd.read_decoded(100) is not None and len(rd.scores()[0]) == 0
    rd.close()
    for bad in ([("NM", "f", 1.0)], [("NM", "A", "3")]):
        bamio.write_bam(path, REFS, recs[:1], tags=[bad])
        with pytest.raises(ValueError, match="not an integer"):
            _native_scores(path, "NM", None, how)


def _truncations(rec, tags):
    """The record ``rec`` (bytes, with tags) cut short inside an aux field, at every byte that is not a field boundary."""
    body = rec[4:]
    start = len(body) - len(bamio.pack_tags(tags))
    ends = {start + len(bamio.pack_tags(tags[:k])) for k in range(len(tags) + 1)}
    return [struct.pack("<i", c) + body[:c] for c in range(start, len(body)) if c not in ends]


def test_the_aux_walk_under_sanitizers_as_a_plain_c_program(tmp_path):
    """``bamdec.c`` and ``tests/bamdec_score_smoke.c`` compiled together under ASAN + UBSAN and run as an executable: the scores of the
    files above, and ``BD_ERR_FORMAT`` -- from every kind of read call, with a clean sanitizer exit -- for copies whose last record
    is cut short inside an aux field, at every byte."""
    from alntools_amd import build as b
    cc = os.path.join(os.path.dirname(os.path.realpath(b.HIPCC)), "..", "lib", "llvm", "bin", "clang")      # (its sanitizer runtimes are linked in)
    if not os.path.exists(cc):
        cc = "/opt/rocm/lib/llvm/bin/clang"
    exe = str(tmp_path / "score_smoke")
    subprocess.check_call([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c11", "-D_POSIX_C_SOURCE=200809L",
                           "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "bamdec_score_smoke.c"), os.path.join(ROOT, "alntools_amd", "csrc", "bamdec.c"),
                           "-o", exe, "-lz", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    recs, tags, want = _scored_records()
    good = str(tmp_path / "scored.bam")
    bamio.write_bam(good, REFS, recs, tags=tags)

    def run(*args):
        out = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
        assert out.returncode == 0 and out.stdout.endswith("score ok\n") and "ERROR" not in out.stderr and "runtime error" not in out.stderr, \
            (args[:3], out.returncode, out.stdout[-500:], out.stderr[-2000:])
        return out.stdout
    for (a, b), w in want.items():
        lines = run("ok", a, b or "-", good).splitlines()[:-1]
        assert [tuple(int(x) for x in l.split()[2:]) for l in lines] == w and [int(l.split()[1]) for l in lines] == list(range(len(recs)))
    cut = []
    raw = [bamio.pack_record(*r, tags=t) for r, t in zip(recs, tags)]
    for last in (0, 3, len(recs) - 1):                       # the last record: one with every type around the tag, the unmapped one
        for k, short in enumerate(_truncations(raw[last], tags[last])):
            path = str(tmp_path / ("cut_%d_%d.bam" % (last, k)))
            _write_raw(path, REFS, raw[:last] + [short])
            cut.append(path)
            if k % 9 == 0:
                with pytest.raises(ValueError):
                    _py_scores(path, "NM", None)
    assert len(cut) > 150
    run("format", "NM", "-", *cut)
    run("format", "AS", "YS", *cut[::7])
    # a record whose CIGAR and sequence lengths point past its end
    body = bytearray(bamio.pack_record(*recs[0], tags=tags[0])[4:])
    body[16:20] = struct.pack("<i", 1 << 20)
    bad = str(tmp_path / "seq.bam")
    _write_raw(bad, REFS, [struct.pack("<i", len(body)) + bytes(body)])
    run("format", "NM", "-", bad)


# ---- the batch cut ------------------------------------------------------------------------------------------------------------------------
def test_batches_are_cut_into_whole_reads():
    rng = np.random.default_rng(7)
    rid = np.concatenate([[NONE] * 2, np.repeat(np.arange(12), rng.integers(1, 6, size=12))]).astype(np.uint32)
    assert es.cut_whole_reads(rid[:0]) == 0 and es.cut_whole_reads(rid[:2]) == 0 and es.cut_whole_reads(rid[:2], final=True) == 2
    assert es.cut_whole_reads(np.array([NONE, NONE, 0, 0, 1, 1, 1], dtype=np.uint32)) == 4
    for size in range(1, 10):
        held, pieces = rid[:0], []
        for lo in range(0, len(rid), size):
            part = np.concatenate([held, rid[lo:lo + size]])
            k = es.cut_whole_reads(part, final=lo + size >= len(rid))
            pieces.append(part[:k])
            held = part[k:]
        assert len(held) == 0 and np.array_equal(np.concatenate(pieces), rid)
        whole = [p for p in pieces if len(p)]                # whole reads: no id in two pieces
        assert all(a[-1] != b[0] for a, b in zip(whole, whole[1:]))


def test_the_feed_carries_the_open_read(monkeypatch):
    """``BestStrata.feed`` with the GPU call replaced by the checker: batches of every size give what one call over the stream gives."""
    from alntools_amd import bam_utils
    rng = np.random.default_rng(8)
    n = 60
    head = rng.random(n) < 0.4
    head[0] = False
    rid = (np.cumsum(head) - 1).astype(np.int64)
    rid = np.where(rid < 0, NONE, rid).astype(np.uint32)
    hf = np.where((rng.random(n) < 0.8) | head, P, F).astype(np.uint32)
    sc = rng.integers(0, 3, size=n).astype(np.int32)
    want = sk.best_strata(rid, hf, sc)
    monkeypatch.setattr(es, "best_strata", lambda r, h, s, lowest=True, device=0: sk.best_strata(r, h, s, lowest))
    for size in range(1, 10):
        st = bam_utils.BestStrata("NM")
        got = []
        for lo in range(0, n, size):
            t = dict(read_id=rid[lo:lo + size], locus=np.arange(lo, min(lo + size, n)), hapflag=hf[lo:lo + size], pos=np.arange(lo, min(lo + size, n)),
                     score=sc[lo:lo + size])
            got.append(st.feed(t))
        got.append(st.finish())
        got = [g for g in got if g is not None]
        assert np.array_equal(np.concatenate([g["read_id"] for g in got]), want[0]) and np.array_equal(np.concatenate([g["hapflag"] for g in got]), want[1])
        assert np.array_equal(np.concatenate([g["locus"] for g in got]), np.arange(n)) and tuple(st.counts) == want[2]


# ---- the command line's refusals -----------------------------------------------------------------------------------------------------------
def _cli(args, env=None):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("ALNTOOLS_GPUS", None)
    e.update(env or {})
    return subprocess.run([sys.executable, "-m", "alntools_amd.cli"] + args, capture_output=True, text=True, env=e, cwd=ROOT)


def test_the_command_lines_refusals(tmp_path):
    recs, tags, _ = _scored_records()
    bam, out = str(tmp_path / "in.bam"), str(tmp_path / "out.bin")
    bamio.write_bam(bam, REFS, recs, tags=tags)
    for cmd, target in (("bam2ec", out), ("bam2emase", str(tmp_path / "out.h5"))):
        r = _cli([cmd, bam, target, "--best-strata", "XS"])
        assert r.returncode == 1 and r.stderr.strip() == "Error: --best-strata XS: the tag is one of NM, XM, nM, AS, AS+YS", (r.stdout, r.stderr)
        r = _cli([cmd, bam, target, "--best-strata", "NM", "--multisample"], env={"ALNTOOLS_GPUS": "2"})
        assert r.returncode == 1 and r.stderr.strip() == "Error: --best-strata does not run with ALNTOOLS_GPUS above 1", (r.stdout, r.stderr)
        r = _cli([cmd, bam, target, "--best-strata", "NM"], env={"ALNTOOLS_GPUS": "2"})
        assert r.returncode == 1 and r.stderr.strip() == "Error: --best-strata does not run with ALNTOOLS_GPUS above 1", (r.stdout, r.stderr)
        for decoder in ("c", "py"):                         # record 10 is the first passing record without NM; AS is missing from record 0 on
            for tag, rec, name in (("NM", 10, "NM"), ("AS", 0, "AS"), ("AS+YS", 0, "AS")):
                r = _cli([cmd, bam, target, "--best-strata", tag], env={"ALNTOOLS_DECODER": decoder})
                assert r.returncode == 1 and r.stderr.strip().splitlines()[-1] == "Error: %s record %d: no %s tag" % (bam, rec, name), (r.stdout, r.stderr)
        assert not os.path.exists(target)
    # the same through the functions: refused before a file is opened (there is none)
    from alntools_amd import bam_utils, bam_utils_multisample, methods
    with pytest.raises(bam_utils.BestStrataError, match="the tag is one of"):
        methods.bam2ec(str(tmp_path / "none.bam"), out, best_strata="as")
    with pytest.raises(bam_utils.BestStrataError, match="the tag is one of"):
        bam_utils_multisample.convert_files([str(tmp_path / "none.bam")], out, None, best_strata="NM+XM")
    assert es.parse_tag("AS+YS") == ("AS", "YS", False) and es.parse_tag("nM") == ("nM", None, True)
