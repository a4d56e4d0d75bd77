"""``--collapse-umis`` without a GPU: the rule's checker against a hand-written dozen of records, a UMI's code, the UMI of every run
through the writer, the Python reader and the native decoder (and the decoder's field walk under sanitizers, as a plain C program), the
binding's tables, and every refusal of the command line.  The GPU side is ``tests/test_gpu_collapse_umis.py``."""
import os
import subprocess

import numpy as np
import pytest

from alntools_amd import bamdec, bamio, bam_utils, bam_utils_multisample as bum, ecb, ecb_umi as eu

import umi_checker as uc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
NONE32 = 0xFFFFFFFF
P, F = 0x0, 0x4
A, B = 77, 78                              # two molecule keys


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------
#          id    locus  hapflag
DOZEN = [(NONE32, 9, F),                   # in front of the stream, carrying the id before read 0's: no read's
         (0, 1, P), (0, 1, P), (0, 2, P | 1 << 16),          # read 0, key A: names (1, 0) twice
         (1, 2, P | 1 << 16), (1, 1, F), (1, 3, P),          # read 1, key A: lacks (1, 0) -- its record of locus 1 does not pass
         (2, 5, P),                        # read 2, key B
         (3, 5, P | 1 << 16),              # read 3, key B: the other haplotype, the intersection is empty
         (4, 7, P), (4, 7, P),             # read 4, no UMI: a molecule of its own, its duplicate kept
         (5, 7, P)]                        # read 5, no UMI: never joins read 4
KEYS = [A, A, B, B, uc.UMI_NONE, uc.UMI_NONE]


def _dozen():
    return tuple(np.array([r[k] for r in DOZEN], dtype=np.uint32) for k in range(3))


def test_the_checker_on_a_hand_written_dozen():
    rid, loc, hf = _dozen()
    assert len(rid) == 12 and uc.breach(rid, loc, hf, 6, 8, 2) is None
    out_id, out_loc, out_hf, first, counts = uc.collapse(rid, loc, hf, KEYS)
    assert out_id.tolist() == [0, 1, 1, 2] and out_loc.tolist() == [2, 7, 7, 7] and out_hf.tolist() == [1 << 16, 0, 0, 0]
    assert first.tolist() == [0, 4, 5]
    assert counts == (6, 4, 2, 1, 4, 2)            # reads, molecules, of several reads, discarded, records out, reads without a UMI
    assert [len(r) for r in uc.reads_of(rid, hf)] == [3, 3, 1, 1, 2, 1]
    # a key of its own for every read: the passing records as they are, the ids from 0
    alone = uc.collapse(rid, loc, hf, [1, 2, 3, 4, 5, 6])
    keep = [i for i, r in enumerate(DOZEN) if uc.passes(r[2])]
    assert alone[0].tolist() == [DOZEN[i][0] for i in keep] and alone[1].tolist() == [DOZEN[i][1] for i in keep] and alone[4] == (6, 6, 0, 0, 10, 0)
    # one molecule of reads 0, 1 and a third that names (2, 1) with flag bits set: emitted with all flag bits zero, ascending
    ids = np.array([NONE32, 0, 0, 0, 1, 1, 1, 2, 2, 3], np.uint32)
    three = uc.collapse(ids, np.array([9, 1, 1, 2, 2, 1, 3, 3, 2, 4], np.uint32), np.array([F, P, P, 1 << 16, 1 << 16, F, P, 0x10, 0x10 | 1 << 16, 0x10], np.uint32), [A, A, A, 5])[:4]
    assert [x.tolist() for x in three] == [[0, 1], [2, 4], [1 << 16, 0x10], [0, 3]]
    # the breaches the library names
    assert uc.breach([0, 1, 1, 0], [0] * 4, [P] * 4, 2, 8, 2) == (3, "read_id falls")
    assert uc.breach([0, 0, 2], [0] * 3, [P] * 3, 2, 8, 2) == (2, "read_id steps by more than 1")
    assert uc.breach([NONE32, 0, 1], [0] * 3, [F, P, F], 2, 8, 2) == (2, "read_id steps on a record that does not pass the filter")
    assert uc.breach([0, 0], [0, 8], [P, P], 1, 8, 2) == (1, "locus at or beyond n_loci")
    assert uc.breach([0, 0], [0, 8], [P, F], 1, 8, 2) is None
    assert uc.breach([0, 0], [0, 0], [P, 2 << 16], 1, 8, 2) == (1, "haplotype at or beyond n_haps")
    assert uc.breach(rid, loc, hf, 5, 8, 2) == (11, "the stream holds 6 reads, n_reads is 5")
    assert uc.breach(rid, loc, hf, 2, 8, 2) == (7, "the stream holds 6 reads, n_reads is 2")
    assert uc.breach(rid, loc, hf, 7, 8, 2) == (11, "the stream holds 6 reads, n_reads is 7")


def test_the_filter_is_the_tuple_contracts():
    from alntools_amd import tuples
    flags = np.arange(0, 0x1000, dtype=np.int64)
    for tid, ntid, npos, bits in ((3, 3, 5, 0), (3, 4, 5, 0x1000), (3, 3, -1, 0x2000), (3, 4, -1, 0x3000)):
        n = len(flags)
        want = tuples.record_valid(flags, np.full(n, tid), np.full(n, ntid), np.full(n, npos))
        assert [uc.passes(int(f) | bits | (5 << 16)) for f in flags] == want.tolist()


# ---- a UMI's code ---------------------------------------------------------------------------------------------------------------------------
def test_pack_umi_on_every_class_of_input():
    assert eu.pack_umi("A") == 0b100 and eu.pack_umi("T") == 0b111 and eu.pack_umi("ACGT") == 0b100011011
    assert eu.pack_umi("AA") != eu.pack_umi("A") != eu.pack_umi("AAA")                 # the leading 1 bit tells the lengths apart
    assert eu.pack_umi("T" * 16) == (1 << 33) - 1 and eu.pack_umi("A" * 16) == 1 << 32
    assert eu.pack_umi(b"AC") == eu.pack_umi("AC") == 0b10001
    for bad in ("", "N", "ACGN", "acgt", "ACgT", "A" * 17, "x6", "AC GT", "AC-GT", None, 5, b"\xff"):
        assert eu.pack_umi(bad) is None, bad
    seen = {eu.pack_umi("".join("ACGT"[(i >> (2 * k)) & 3] for k in range(n))) for n in range(1, 5) for i in range(4 ** n)}
    assert len(seen) == 4 + 16 + 64 + 256 and None not in seen
    keys = eu.mol_keys([3, 3, 0, (1 << 22) - 1, 5], ["AC", "AN", "T" * 16, "T" * 16, ""])
    assert keys.dtype == np.uint64 and keys.tolist() == [3 << 33 | 0b10001, eu.UMI_NONE, (1 << 33) - 1, ((1 << 22) - 1) << 33 | ((1 << 33) - 1), eu.UMI_NONE]
    assert eu.UMI_NONE == uc.UMI_NONE == (1 << 64) - 1 and max(keys.tolist()[2:4]) < eu.UMI_NONE and eu.MAX_RECORDS == (1 << 30) - 1


def test_the_binding_has_tables_of_its_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_umi.h")).read()
    import re
    assert set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M)) == set(eu.UMI_SYMBOLS) == {"ecb_collapse_umis", "ecb_collapse_umis_device"}
    assert [(s[0], len(s[1]), s[3]) for s in eu.UMI_SIGNATURES] == [("ecb_collapse_umis", 14, True)]
    assert not set(eu.UMI_SYMBOLS) & set(ecb.SYMBOLS) and '"ecb_umi.h"' in open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert "#define ECB_UMI_NONE 0xFFFFFFFFFFFFFFFFull" in hdr
    assert issubclass(eu.UmiContractError, ecb.EcbError) and eu.UmiContractError(-5, "umi: record 3: x", 3).record == 3
    lib = os.path.join(ROOT, "alntools_amd", "libecb.so")
    if os.path.exists(lib):                                  # the built library exports both
        import ctypes
        so = ctypes.CDLL(lib)
        for name in eu.UMI_SYMBOLS:
            assert hasattr(so, name), name


# ---- the UMI of every run -----------------------------------------------------------------------------------------------------------------
REFS = [("T0_A", 1000), ("T0_B", 1000)]


def _name(read, cell, umi, fields=15):
    f = ["x%d" % k for k in range(fields)]
    f[0] = read
    if fields > 6:
        f[6] = umi
    if fields > 14:
        f[14] = cell
    return "|||".join(f)


def _runs():
    """-> (records, the (cell, umi) of every run): names with and without a space, UMIs that are none."""
    recs, runs = [], []
    umis = ["ACGT", "", "ACGTACGTACGTACGT", "A" * 17, "acgt", "ACGN", "T", "GATTACA", "x6", "AC GT"]
    for r in range(40):
        cell, umi = "BC%d" % (r % 3), umis[r % len(umis)]
        name = _name("r%03d" % r, cell, umi)
        if r % 7 == 3:
            name += " 1:N:0"                                  # tracked untrimmed after a switch: every record of it is a run of its own
        n_rec = 1 + r % 3
        for k in range(n_rec):
            recs.append((name, 4 if k == 1 else 0, k % 2, 10 + r, -1, -1))
        n_valid = n_rec - (1 if n_rec > 1 else 0)
        f = name.split("|||")                               # (a spaced name is tracked whole: its last field keeps what follows the space)
        runs += [(f[14], f[6])] * (n_valid if " " in name else 1)
    return recs, runs


def _scan(path, decoder, batch):
    old = bam_utils.BATCH_RECORDS, bum.BATCH_RECORDS
    bam_utils.BATCH_RECORDS = bum.BATCH_RECORDS = batch
    try:
        rd = bamio.BamReader(path) if decoder == "py" else bamdec.NativeBamReader(path, threads=2)
        try:
            return bum.scan_file(rd, None, umis=True), bum.scan_file(bamio.BamReader(path), None)
        finally:
            rd.close()
    finally:
        bam_utils.BATCH_RECORDS, bum.BATCH_RECORDS = old


@pytest.mark.parametrize("decoder", ["py", "c"])
def test_the_umi_of_every_run_under_both_decoders(tmp_path, decoder):
    bamdec.build()
    recs, runs = _runs()
    path = str(tmp_path / "umis.bam")
    bamio.write_bam(path, REFS, recs)
    for batch in (3, 7, 1000):
        with_umis, plain = _scan(path, decoder, batch)
        c, keep, cells, ctr, umis = with_umis
        assert len(cells) == len(umis) == len(runs) - 1 and list(zip(cells, umis)) == runs[:-1], batch      # (the file's last run is never counted)
        # next to the cells: nothing else changes
        assert cells == plain[2] and ctr == plain[3] and np.array_equal(keep, plain[1]) and all(np.array_equal(c[k], plain[0][k]) for k in plain[0])
    if decoder == "c":                                       # off, as a handle starts: four values, no UMIs kept
        rd = bamdec.NativeBamReader(path)
        assert len(bum.scan_file(rd, None)) == 4 and rd.ms_umis() == []
        rd.close()
        rd = bamdec.NativeBamReader(path)
        rd.set_umi(True)
        d, cells = rd.read_ms(1000)
        assert len(rd.ms_umis()) == len(cells) == len(runs)
        rd.set_umi(False)
        assert rd.ms_umis() == []
        rd.close()


def _cut_names():
    """A full name cut short at every byte: -> [(name, (cell, umi) or None where field 14 is missing)]"""
    full = _name("r1", "CELL", "ACGTAC")
    out = []
    for c in range(1, len(full) + 1):
        f = full[:c].split("|||")
        out.append((full[:c], (f[14], f[6]) if len(f) >= 15 else None))
    assert sum(1 for _, w in out if w is not None) == 5 and len(out) > 60
    for umi in ("", "A" * 17, "A" * 16, "N"):
        out.append((_name("r2", "C", umi), ("C", umi)))
    out.append((_name("r3", "", "AC"), ("", "AC")))
    out.append(("|||" * 14, ("", "")))
    out.append(("|||" * 13 + "||", None))
    out.append(("|", None))
    return out


def test_the_field_walk_under_sanitizers_as_a_plain_c_program(tmp_path):
    """``bamdec.c`` and ``tests/bamdec_umi_smoke.c`` compiled together under ASAN + UBSAN and run as an executable: the cell and the UMI
    of every run of the file above, of names cut short inside every field -- ``BD_ERR_FORMAT`` where field 14 is gone, with a clean
    sanitizer exit -- and of names whose field 6 is empty or 17 bases long.  The Python reader says the same of every file."""
    from alntools_amd import build as b
    cc = os.path.join(os.path.dirname(os.path.realpath(b.HIPCC)), "..", "lib", "llvm", "bin", "clang")      # (its sanitizer runtimes are linked in)
    if not os.path.exists(cc):
        cc = "/opt/rocm/lib/llvm/bin/clang"
    exe = str(tmp_path / "umi_smoke")
    subprocess.check_call([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c11", "-D_POSIX_C_SOURCE=200809L",
                           "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "bamdec_umi_smoke.c"), os.path.join(ROOT, "alntools_amd", "csrc", "bamdec.c"),
                           "-o", exe, "-lz", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        out = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
        assert out.returncode == 0 and out.stdout.endswith("umi ok\n") and "ERROR" not in out.stderr and "runtime error" not in out.stderr, \
            (args[:3], out.returncode, out.stdout[-500:], out.stderr[-2000:])
        return out.stdout.splitlines()[:-1]
    recs, runs = _runs()
    good = str(tmp_path / "umis.bam")
    bamio.write_bam(good, REFS, recs)
    lines = run("ok", good)
    want = ["%s %d <%s> <%s>" % (good, k, c, u) for k, (c, u) in enumerate(runs)] + ["%s %d <%s>" % (good, k, c) for k, (c, u) in enumerate(runs)]
    assert lines == want
    ok, bad = [], []
    for k, (name, w) in enumerate(_cut_names()):
        path = str(tmp_path / ("cut_%03d.bam" % k))
        # the cut name starts the second run: the walk then sees the whole (untrimmed) name; a plain read follows, so that run is counted
        bamio.write_bam(path, REFS, [(_name("r0", "C0", "GG"), 0, 0, 1, -1, -1), (name, 0, 0, 2, -1, -1), (_name("r9", "C9", "TT"), 0, 1, 3, -1, -1)])
        (ok if w is not None else bad).append((path, w))
        rd = bamio.BamReader(path)
        if w is None:
            with pytest.raises(ValueError):
                bum.scan_file(rd, None, umis=True)
        else:
            got = bum.scan_file(rd, None, umis=True)
            assert (got[2], got[4]) == (["C0", w[0]], ["GG", w[1]]), name
        rd.close()
    lines = run("ok", *[p for p, _ in ok])
    want = [l for p, w in ok for l in ("%s 0 <C0> <GG>" % p, "%s 1 <%s> <%s>" % (p, w[0], w[1]), "%s 2 <C9> <TT>" % p)]
    assert [l for l in lines if l.count("<") == 2] == want
    run("format", *[p for p, _ in bad])


# ---- the command line's refusals -----------------------------------------------------------------------------------------------------------
def test_the_command_lines_refusals(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods, utils
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    src = str(tmp_path / "dir")
    os.makedirs(src)
    bamio.write_bam(os.path.join(src, "a.bam"), REFS, _runs()[0])

    def refused(args, env=None):
        level = utils.get_logger().level
        try:
            r = CliRunner().invoke(cli.cli, args, env=env)
        finally:
            utils.get_logger().setLevel(level)              # (the command sets the package's log level: later tests find it as it was)
        assert r.exit_code == 1 and r.output.startswith("Error: --collapse-umis") and len(r.output.strip().splitlines()) == 1, (args, r.exit_code, r.output)
        return r.output.strip()
    for cmd, target in (("bam2ec", str(tmp_path / "out.bin")), ("bam2emase", str(tmp_path / "out.h5"))):
        assert refused([cmd, os.path.join(src, "a.bam"), target, "--collapse-umis"]) == \
            "Error: --collapse-umis needs --multisample: the cell and the UMI are fields of the multisample read names"
        assert refused([cmd, src, target, "--multisample", "--collapse-umis", "--rangefile", str(tmp_path / "r.txt")]) == \
            "Error: --collapse-umis does not run with --rangefile: the ranges are defined over alignments that the collapse removes"
        assert refused([cmd, src, target, "--multisample", "--collapse-umis"], env={"ALNTOOLS_GPUS": "2"}) == \
            "Error: --collapse-umis does not run with ALNTOOLS_GPUS above 1"
        assert not os.path.exists(target) and not os.path.exists(str(tmp_path / "r.txt"))
    # the same through the functions: refused before a file is opened (there is none)
    with pytest.raises(bum.CollapseUmisError, match="--collapse-umis does not run with --rangefile"):
        methods.bam2ec_multisample(str(tmp_path / "nowhere"), str(tmp_path / "o.bin"), range_filename=str(tmp_path / "r.txt"), collapse_umis=True)
    monkeypatch.setenv("ALNTOOLS_GPUS", "4")
    with pytest.raises(bum.CollapseUmisError, match="--collapse-umis does not run with ALNTOOLS_GPUS above 1"):
        bum.convert_files([str(tmp_path / "none.bam")], str(tmp_path / "o.bin"), None, collapse_umis=True)
    monkeypatch.delenv("ALNTOOLS_GPUS")
    # more records than one call collapses: refused by name where the run's records are gathered, before the GPU sees one
    g = bum._Gather()
    most = np.broadcast_to(np.uint32(0), (eu.MAX_RECORDS,))
    g.push(most, most, most)
    with pytest.raises(bum.CollapseUmisError, match=r"--collapse-umis: more than 1,073,741,823 records in the run"):
        g.push(most[:1], most[:1], most[:1])
    # ... which the command line reports as it reports the others
    with pytest.raises(SystemExit):
        with cli._strata_errors():
            raise bum.CollapseUmisError("--collapse-umis: more than 1,073,741,823 records in the run")
    # without the option the keyword is not passed at all: the call is today's
    assert cli._umi_option(False, False, "r.txt") == {} and cli._umi_option(True, True, None) == {"collapse_umis": True}
