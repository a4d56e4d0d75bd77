"""bus2ec on the CPU: the checker (``tests/bus_checker.py``) held to a hand-written case whose expected A, N and samples are spelled out here,
the 2-bit coding both ways, every host-side refusal with its file and line, the ``matrix.ec`` parser against a per-line parse, and
``bus_from_bin`` followed by the checker against the golden ``.bin`` files."""
import logging
import os

import numpy as np
import pytest

from alntools_amd import bin_utils, bus_utils

import bus_checker as bc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the hand-written case ------------------------------------------------------------------------------------------------------------------
NAMES = ["g1_A", "g1_B", "g2_A", "g3_A"]                     # transcripts g1, g2, g3; haplotypes A, B
TCOL, THAP = [0, 0, 1, 2], [0, 1, 0, 0]
LINES = [[0], [0, 1], [0, 1, 2], [1, 2, 3], [3], [0, 2, 3]]
AC, GT = 1, 11
HAND = [   # barcode, UMI, ec, count
    (GT, 5, 1, 2),      # a molecule of one EC: a read of line 1 in GT
    (AC, 0, 2, 1),      # (AC, 0) names lines 2 and 1: {0,1,2} & {0,1} = {0,1}, the set of line 1 -- a new row that joins line 1's EC
    (AC, 0, 1, 1),
    (AC, 3, 2, 1),      # (AC, 3) names lines 2, 3 and 5: {0,1,2} & {1,2,3} & {0,2,3} = {2} -- founds a new EC
    (AC, 3, 3, 4),
    (AC, 3, 5, 1),
    (AC, 7, 0, 1),      # (AC, 7) names lines 0 and 4: {0} & {3} is empty -- discarded
    (AC, 7, 4, 1),
    (GT, 5, 1, 2),      # the first record again
    (GT, 3, 2, 1),      # UMI 3 in another cell: a molecule of its own, a read of line 2
    (AC, 9, 4, 3),      # line 4 in both cells
    (GT, 9, 4, 1),
]


def _hand():
    return bc.records(*[np.array([r[k] for r in HAND], dtype=np.uint64 if k < 2 else np.int64) for k in range(4)])


def _same(res, A, N, samples):
    for got, want in zip(res.A + res.N, A + N):
        assert np.array_equal(got, np.array(want)), (got, want)
    assert res.samples == samples


def test_the_checker_on_the_hand_written_case():
    res = bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, mincount=1)
    # ECs: line 1 ((g1: A|B)), line 2 ((g1: A|B), (g2: A)), line 4 ((g3: A)), then the new row ((g2: A))
    _same(res, ([0, 1, 3, 4, 5], [0, 0, 1, 2, 1], [3, 3, 1, 1, 1]), ([0, 3, 6], [0, 2, 3, 0, 1, 2], [1, 1, 1, 1, 1, 1]), ["AC", "GT"])
    assert res.stats == dict(records=12, molecules=7, molecules_in_several_ecs=3, molecules_discarded=1, new_ecs=1, cells=2, cells_kept=2)
    mol = bc.molecules(_hand(), LINES, TCOL, THAP)
    assert mol.barcodes == [AC, GT] and mol.row_line == [1, 2, 4, -1, -1] and mol.sizes == (2, 5, 6, 6, 7, 3, 1, 2)
    assert mol.rows == [((0,), (3,)), ((0, 1), (3, 1)), ((2,), (1,)), ((0,), (3,)), ((1,), (1,))]
    assert mol.N == {(0, 1): 1, (1, 1): 1, (2, 0): 1, (2, 1): 1, (3, 0): 1, (4, 0): 1}


def test_the_checker_without_umis_on_the_same_bytes():
    A = ([0, 1, 2, 4, 7, 8, 11], [0, 0, 0, 1, 0, 1, 2, 2, 0, 1, 2], [1, 3, 3, 1, 2, 1, 1, 1, 1, 1, 1])
    res = bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, mincount=1, no_umi=True)
    _same(res, A, ([0, 6, 9], [0, 1, 2, 3, 4, 5, 1, 2, 4], [1, 1, 2, 4, 4, 1, 4, 1, 1]), ["AC", "GT"])
    assert res.stats["molecules"] == 12 and res.stats["new_ecs"] == 0
    res = bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, mincount=7, no_umi=True)              # GT counts 6 reads: it goes
    _same(res, A, ([0, 6], [0, 1, 2, 3, 4, 5], [1, 1, 2, 4, 4, 1]), ["AC"])
    with pytest.raises(ValueError, match="no sample left"):
        bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, mincount=14, no_umi=True)


def test_the_checker_with_names_keeps_the_files_order_and_only_its_barcodes():
    res = bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, names=[(GT, "late"), (15, "absent"), (AC, "early")], mincount=1)
    _same(res, ([0, 1, 3, 4, 5], [0, 0, 1, 2, 1], [3, 3, 1, 1, 1]), ([0, 3, 6], [0, 1, 2, 0, 2, 3], [1, 1, 1, 1, 1, 1]), ["late", "early"])
    res = bc.bus2ec(_hand(), 2, LINES, TCOL, THAP, names=[(GT, "only")], mincount=0)
    _same(res, ([0, 1, 3, 4], [0, 0, 1, 2], [3, 3, 1, 1]), ([0, 3], [0, 1, 2], [1, 1, 1]), ["only"])
    assert res.stats["records"] == 12 and res.stats["molecules"] == 3


# ---- the 2-bit coding -------------------------------------------------------------------------------------------------------------------------
def test_the_two_bit_coding_both_ways():
    assert bus_utils.encode("A") == 0 and bus_utils.encode("T") == 3 and bus_utils.encode("AC") == AC and bus_utils.encode("GT") == GT
    assert bus_utils.encode("CAT") == 0b010011 and bus_utils.decode(0b010011, 3) == "CAT" and bus_utils.decode(1, 4) == "AAAC"
    top = "T" + "A" * 30 + "C"                                   # 32 bases: the first one sits in bits 63 and 62
    assert bus_utils.encode(top) == (3 << 62) | 1 and bus_utils.decode((3 << 62) | 1, 32) == top
    assert bus_utils.decode(np.uint64((2 << 62) | 3), 32) == "G" + "A" * 30 + "T"
    rng = np.random.default_rng(3)
    for n in (1, 15, 16, 17, 31, 32):
        s = "".join(rng.choice(list("ACGT"), size=n))
        assert bus_utils.decode(bus_utils.encode(s), n) == s == bc.decode(bc.encode(s), n) and bus_utils.encode(s) == bc.encode(s) < 4 ** n
    for bad in ("ACGN", "acgt", "A" * 33):
        with pytest.raises(ValueError):
            bus_utils.encode(bad)


# ---- refusals on the host ---------------------------------------------------------------------------------------------------------------------
def _dir(tmp_path, **kw):
    return bc.write_bus_dir(str(tmp_path / "bus"), kw.pop("rec", _hand()), kw.pop("bclen", 2), kw.pop("umilen", 2), kw.pop("lines", LINES),
                            kw.pop("names", NAMES), **kw)


def _refused(tmp_path, caplog, d, text, **kw):
    out = str(tmp_path / "out.bin")
    with caplog.at_level(logging.ERROR):
        with pytest.raises(ValueError) as e:
            bus_utils.convert(d, out, **kw)
    assert text in str(e.value), str(e.value)
    assert any(r.getMessage().startswith("Error: ") and text in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def test_a_wrong_magic_version_or_length_is_refused(tmp_path, caplog):
    d = _dir(tmp_path, version=2)
    _refused(tmp_path, caplog, d, "output.bus: BUS version 2")
    with open(os.path.join(d, "output.bus"), "r+b") as fh:
        fh.write(b"BAM\1")
    _refused(tmp_path, caplog, d, "output.bus: not a BUS file")
    for kw, text in ((dict(bclen=0), "a barcode length of 0"), (dict(bclen=33), "a barcode length of 33"), (dict(umilen=0), "a UMI length of 0"),
                     (dict(umilen=33), "a UMI length of 33")):
        _refused(tmp_path, caplog, _dir(tmp_path, **kw), "output.bus: " + text)
    _refused(tmp_path, caplog, _dir(tmp_path, umilen=17), "a UMI length of 17; the sort keys hold 16")


def test_a_ragged_or_empty_file_is_refused(tmp_path, caplog):
    d = _dir(tmp_path)
    with open(os.path.join(d, "output.bus"), "ab") as fh:
        fh.write(b"\0" * 31)
    _refused(tmp_path, caplog, d, "output.bus: 463 bytes are not a header of 48 bytes and whole records of 32")
    _refused(tmp_path, caplog, _dir(tmp_path, rec=_hand()[:0]), "output.bus: no records")


def test_too_many_records_are_refused_by_the_size_alone(tmp_path, monkeypatch):
    d = _dir(tmp_path, text=b"")
    path = os.path.join(d, "output.bus")
    assert bus_utils.read_header(path).n_records == 12
    monkeypatch.setattr(bus_utils.os.path, "getsize", lambda p: 20 + 32 * ((1 << 30) - 1))      # (the size is all that is looked at)
    assert bus_utils.read_header(path).n_records == (1 << 30) - 1
    monkeypatch.setattr(bus_utils.os.path, "getsize", lambda p: 20 + 32 * (1 << 30))
    with pytest.raises(ValueError, match=r"output.bus: 1,073,741,824 records; 2\^30 or more"):
        bus_utils.read_header(path)


@pytest.mark.parametrize("text,line,what", [
    ("0\t0\n2\t1\n", 2, "line number 2 out of sequence (expected 1)"),
    ("0\t0\n1\t1,1\n", 2, "target ids not strictly ascending"),
    ("0\t0\n1\t0,1\n2\t2,1\n", 3, "target ids not strictly ascending"),
    ("0\t0\n1\t0,4\n", 2, "target id 4 at or beyond the 4 names"),
    ("0\t0\n\n", 2, "an empty field"),
    ("0\t0\n1\t\n", 2, "an empty field"),
    ("0\t0,\n", 1, "an empty field"),
    ("0\t0\n1,1\n", 2, "not <number><TAB><id>,<id>,..."),
    ("0\t0\t1\n", 1, "not <number><TAB><id>,<id>,..."),
    ("0\t0\n1\t-1\n", 2, "a byte other than a digit, tab, comma or line end"),
    ("0\t0\n1\t12345678901\n", 2, "a number of more than 10 digits"),
])
def test_a_malformed_matrix_ec_is_refused_with_its_line(tmp_path, caplog, text, line, what):
    d = _dir(tmp_path)
    with open(os.path.join(d, "matrix.ec"), "w") as fh:
        fh.write(text)
    _refused(tmp_path, caplog, d, "matrix.ec line %d: %s" % (line, what))


def test_names_lengths_and_targets_are_refused_with_file_and_line(tmp_path, caplog):
    d = _dir(tmp_path)

    def names(text):
        p = str(tmp_path / "names.txt")
        with open(p, "w") as fh:
            fh.write(text)
        return p
    for text, what in (("AC\ta\nACG\tb\n", "names.txt line 2: barcode 'ACG' has 3 bases; the BUS file's have 2"),
                       ("AC\ta\nAN\tb\n", "names.txt line 2: barcode 'AN' has a letter outside ACGT"),
                       ("AC\ta\nGT\tb\nAC\tc\n", "names.txt line 3: barcode 'AC' is listed twice (first on line 1)"),
                       ("AC\ta\nGT\ta\n", "names.txt line 2: name 'a' is listed twice (first on line 1)"),
                       ("AC\ta\nGT\n", "names.txt line 2: not <barcode><TAB><name>")):
        _refused(tmp_path, caplog, d, what, names_file=names(text))
    for text, what in (("g1_A\t10\nzz_A\t3\n", "lengths.txt line 2: target 'zz_A' is not in transcripts.txt"),
                       ("g1_A\t10\ng1_A\t3\n", "lengths.txt line 2: target 'g1_A' is listed twice"),
                       ("g1_A\tten\n", "lengths.txt line 1: length 'ten' is not a number"),
                       ("g1_A\t1\ng1_B\t2147483648\n", "lengths.txt line 2: length '2147483648' is beyond int32"),
                       ("g1_A\t1\n", "lengths.txt: target 'g1_B' of transcripts.txt has no line")):
        p = str(tmp_path / "lengths.txt")
        with open(p, "w") as fh:
            fh.write(text)
        _refused(tmp_path, caplog, d, what, lengths_file=p)
    _refused(tmp_path, caplog, _dir(tmp_path, names=["g1_A", "g1", "g2_A", "g3_A"]), "transcripts.txt line 2: target name 'g1' is not <transcript>_<haplotype>")
    _refused(tmp_path, caplog, _dir(tmp_path, names=["g1_A", "g2_A", "g1_A", "g3_A"]), "transcripts.txt line 3: target name 'g1_A' is listed twice (first on line 1)")
    many = ["t_h%d" % k for k in range(32)]
    _refused(tmp_path, caplog, _dir(tmp_path, names=many), "transcripts.txt: 32 haplotypes; a .bin holds at most 31")


def test_one_haplotype_by_name_takes_every_name_as_a_transcript():
    tr, hp, col, hap = bus_utils.number_bus_targets(["ENST1.2", "a_b_c", "x"], ["x", "extra"], haplotype="ref")
    assert tr == ["ENST1.2", "a_b_c", "x", "extra"] and hp == ["ref"] and col.tolist() == [0, 1, 2] and hap.tolist() == [0, 0, 0]
    tr, hp, col, hap = bus_utils.number_bus_targets(NAMES, ["g9"])
    assert tr == ["g1", "g2", "g3", "g9"] and hp == ["A", "B"] and col.tolist() == TCOL and hap.tolist() == THAP


def test_the_stats_file_has_one_line_per_number():
    s = dict(records=12, molecules=7, molecules_in_several_ecs=3, molecules_discarded=1, new_ecs=1, cells=2, cells_kept=2)
    assert bus_utils.stats_text(s) == ("records\t12\nmolecules\t7\nmolecules_in_several_ecs\t3\nmolecules_discarded\t1\nnew_ecs\t1\ncells\t2\n"
                                       "cells_kept\t2\n")


# ---- the header and the bindings ----------------------------------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_modules_symbols():
    import re
    from alntools_amd import build, ecb, ecb_bus
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "ecb_bus.h")).read()
    declared = re.findall(r"^int (ecb_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(ecb_bus.BUS_SYMBOLS) and len(set(declared)) == 2
    main = open(os.path.join(root, "include", "ecb.h")).read()
    assert len(re.findall(r'^#\s*include "ecb_bus\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and "ABI 4, additive" in text
    bound = [n for name, _, _, twin, _ in ecb_bus.BUS_SIGNATURES for n in ((name + "_device", name) if twin else (name,))]
    assert sorted(bound) == sorted(ecb_bus.BUS_SYMBOLS) and not set(bound) & set(ecb.SYMBOLS)
    for name, argtypes, _, _, _ in ecb_bus.BUS_SIGNATURES:          # as many parameters as the prototypes have
        for n in (name, name + "_device"):
            proto = re.search(r"^int %s\((.*?)\);" % n, text, re.M | re.S).group(1)
            assert len(proto.split(",")) == len(argtypes), n
    assert any(p.endswith("ecb_bus.h") for p in build.inputs()) and any(p.endswith("bus.inc") for p in build.inputs())
    assert len(re.findall(r'^#include "bus\.inc"', open(os.path.join(root, "alntools_amd", "csrc", "ecb.hip")).read(), re.M)) == 1
    assert "ECB_BUS_MAX_UMILEN" in text and "at most n" in text and "A capacity too small is ECB_ERR_ARG" in text


def test_the_command_line_lists_bus2ec_and_imports_no_torch_for_it():
    from alntools_amd import cli, methods
    assert "``bus2ec``" in cli.__doc__ and "``bus2ec``" in methods.__doc__ and "bus2ec" in cli.cli.commands
    opts = {o for p in cli.cli.commands["bus2ec"].params for o in p.opts}
    assert {"--no-umi", "-m", "--names", "-l", "-H", "-t", "--stats", "-v"} <= opts
    assert [p.default for p in cli.cli.commands["bus2ec"].params if "-m" in p.opts] == [1000]


# ---- the matrix.ec parser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_matrix_ec_parser_against_a_per_line_parse(tmp_path, seed):
    rng = np.random.default_rng(seed)
    T = 1500
    lines = [sorted(rng.choice(T, size=int(k), replace=False).tolist()) for k in rng.integers(1, 12, size=400)]
    lines[7] = [int(rng.integers(T))]                            # a line of one target
    lines[250] = list(range(T))                                  # a line of all targets
    lines.append([T - 1])
    p = str(tmp_path / "matrix.ec")
    with open(p, "w") as fh:
        fh.write("".join("%d\t%s\n" % (i, ",".join(map(str, x))) for i, x in enumerate(lines)))
    if seed == 2:
        with open(p, "rb+") as fh:                               # (no line end behind the last line)
            fh.seek(-1, os.SEEK_END)
            fh.truncate()
    want = []
    with open(p) as fh:
        for i, ln in enumerate(fh):
            num, ids = ln.rstrip("\n").split("\t")
            assert int(num) == i
            want.append([int(t) for t in ids.split(",")])
    ptr, ids = bus_utils.parse_matrix_ec(p, T)
    wp, wi = bc.csr_lines(want)
    assert ptr.dtype == ids.dtype == np.uint32 and np.array_equal(ptr, wp) and np.array_equal(ids, wi)


# ---- a .bin as a BUS directory, and back ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("g4_multi_min0", {}), ("g4b_multi_min0", {}), ("g4b_multi_min0", dict(split=True, shuffle=True)),
                                          ("g4_multi_min0", dict(no_umi=True)), ("g4_multi_min0", dict(split=True, triple=True))],
                         ids=["g4", "g4b", "g4b-split-shuffled", "g4-no-umi", "g4-split-tripled"])
def test_bus_from_bin_and_the_checker_give_the_golden_bin_back(tmp_path, name, variant):
    m = bin_utils.ecload(os.path.join(GOLDEN, name + ".bin"))
    b = bc.bus_from_bin(m, str(tmp_path / "bus"), seed=5, **variant)
    hdr = bus_utils.read_header(os.path.join(b["dir"], "output.bus"))
    rec = bus_utils.read_records(os.path.join(b["dir"], "output.bus"), hdr)
    assert (hdr.bclen, hdr.umilen, hdr.n_records) == (16, 12, len(b["records"])) and np.array_equal(rec, b["records"])
    names = bus_utils.read_transcripts(os.path.join(b["dir"], "transcripts.txt"))
    tr, hp, col, hap = bus_utils.number_bus_targets(names)
    assert tr == m.lname and hp == m.hname
    ptr, ids = bus_utils.parse_matrix_ec(os.path.join(b["dir"], "matrix.ec"), len(names))
    lines = [ids[ptr[i]:ptr[i + 1]].tolist() for i in range(len(ptr) - 1)]
    assert lines == b["lines"] and (len(lines) > m.num_reads) == bool(variant.get("split"))
    values, snames = bus_utils.read_names(b["names"], hdr.bclen)
    assert snames == m.sname and not np.array_equal(values, np.sort(values))
    lengths = np.zeros_like(m.lengths)
    lengths[col, hap] = bus_utils.read_lengths(b["lengths"], names)
    assert np.array_equal(lengths, m.lengths)
    res = bc.bus2ec(rec, hdr.bclen, lines, col, hap, names=list(zip(values.tolist(), snames)), mincount=0, no_umi=bool(variant.get("no_umi")))
    assert res.samples == m.sname
    for got, want in zip(res.A + res.N, (m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN)):
        assert np.array_equal(got, want)
    if variant.get("split"):
        assert res.stats["molecules_in_several_ecs"] > 100 and res.stats["new_ecs"] == 0 and res.stats["molecules_discarded"] == 0
