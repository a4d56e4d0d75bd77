"""salmon2ec on the host (no GPU): the header, quant.sf and -t parsing and every host-side refusal; the numpy checker against every
reference golden byte for byte; the .gz file read as the plain one."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest

from alntools_amd import bin_utils, salmon_utils

import salmon_checker as chk


def _cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, "salmon_cases.json")))


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _checker_bytes(golden_dir, c):
    d = os.path.join(golden_dir, c["dir"])
    tf = os.path.join(d, c["targets"]) if c["targets"] else None
    h, l, lens, ip, ix, da, np_, nx, nd = chk.expected_from_dir(d, tf)
    return bin_utils.ecsave2_bytes(bin_utils.ECMatrices(h, l, lens, [c["sample"]], ip, ix, da, np_, nx, nd))


def test_checker_reproduces_every_reference_golden(golden_dir):
    done = 0
    for c in _cases(golden_dir):
        if c["bin"] is None or c["name"].startswith("dev_"):
            continue
        assert _checker_bytes(golden_dir, c) == _bytes(os.path.join(golden_dir, c["bin"])), c["name"]
        done += 1
    assert done == 7


@pytest.mark.parametrize("name,line,reason", [("dev_k", 1, chk.R_K), ("dev_repeat", 1, chk.R_REPEAT), ("dev_fewer", 2, chk.R_COUNT),
                                              ("err_more_lines", 2, chk.R_COUNT), ("err_target_id", 1, chk.R_TARGET),
                                              ("err_letter", 1, chk.R_BYTE), ("err_empty_line", 1, chk.R_EMPTY),
                                              ("err_empty_field", 1, chk.R_EMPTY)])
def test_checker_refuses_the_malformed_ec_sections(golden_dir, name, line, reason):
    with pytest.raises(chk.Refusal) as e:
        chk.expected_from_dir(os.path.join(golden_dir, "salmon_" + name))
    assert (e.value.line, e.value.reason) == (line, reason)


def test_header_parse_and_numbering():
    data = b"4\r\n3\n T1_B \nT1_A\r\nT0_B\nT0_A\n2\t0\t1\t5\n"
    h = salmon_utils.parse_header(data)
    assert (h.n_targets, h.n_ecs, h.n_lines) == (4, 3, 6)
    assert h.names == [" T1_B", "T1_A", "T0_B", "T0_A"]
    assert data[h.ec_offset:] == b"2\t0\t1\t5\n"
    tx, hp, col, hap = salmon_utils.number_targets(h.names[1:], ["T9", "T1", "T0", "T8"])
    assert tx == ["T1", "T0", "T9", "T8"] and hp == ["A", "B"]
    assert col.tolist() == [0, 1, 1] and hap.tolist() == [0, 1, 0]
    h = salmon_utils.parse_header(b"1\n0\nT1_A")                        # (the last name ends the file)
    assert h.names == ["T1_A"] and h.ec_offset == len(b"1\n0\nT1_A")


@pytest.mark.parametrize("data,msg", [(b"x\n1\n", "line 1: the number of targets is not an integer"),
                                      (b"1\n", "ends before the number of ECs"),
                                      (b"3\n1\nA_B\nC_D\n", "lists 2 target names, fewer than T = 3"),
                                      (b"2\n-1\nA_B\nC_D\n", "line 2: a negative count")])
def test_header_refusals(data, msg):
    with pytest.raises(ValueError, match=msg):
        salmon_utils.parse_header(data, "eq")


@pytest.mark.parametrize("names,msg", [(["T1_A", "T1B"], "line 4: target name 'T1B' is not <transcript>_<haplotype>"),
                                       (["T1_A", "T1_B_C"], "line 4: target name 'T1_B_C'"),
                                       (["T1_A", "T2_A", "T1_A"], "line 5: target name 'T1_A' is listed twice \\(first on line 3\\)")])
def test_name_refusals(names, msg):
    with pytest.raises(ValueError, match=msg):
        salmon_utils.number_targets(names, (), "eq")


def _quant(tmp_path, rows):
    p = str(tmp_path / "quant.sf")
    with open(p, "w") as f:
        f.write("Name\tLength\tEffectiveLength\tTPM\tNumReads\n" + "".join(r + "\n" for r in rows))
    return p


def test_lengths_truncate_toward_zero(tmp_path):
    p = _quant(tmp_path, ["B_1\t9\t0.5\t1\t1", "A_1\t9\t80.7\t1\t1\r", "C_1\t9\t-0.9\t1\t1", "D_1\t9\t1e3\t1\t1"])
    assert salmon_utils.read_lengths(p, ["A_1", "B_1", "C_1", "D_1"]).tolist() == [80, 0, 0, 1000]


@pytest.mark.parametrize("rows,msg", [(["A_1\t9\t1\t1\t1"], "target 'B_1' of the eq_classes header has no line"),
                                      (["A_1\t9\t1", "B_1\t9\t1", "Z_1\t9\t1"], "line 4: target 'Z_1' is not in the eq_classes header"),
                                      (["A_1\t9\t1", "B_1\t9\t1", "A_1\t9\t2"], "line 4: target 'A_1' is listed twice"),
                                      (["A_1\t9", "B_1\t9\t1"], "line 2: no EffectiveLength column"),
                                      (["A_1\t9\tabc", "B_1\t9\t1"], "line 2: EffectiveLength 'abc' is not a number"),
                                      (["A_1\t9\t3e9", "B_1\t9\t1"], "line 2: EffectiveLength '3e9' is beyond int32"),
                                      (["A_1\t9\tnan", "B_1\t9\t1"], "beyond int32")])
def test_quant_refusals(tmp_path, rows, msg):
    with pytest.raises(ValueError, match=msg):
        salmon_utils.read_lengths(_quant(tmp_path, rows), ["A_1", "B_1"])


def test_targets_file_as_the_reference_reads_it(tmp_path):
    p = str(tmp_path / "t.tsv")
    with open(p, "w") as f:
        f.write("T9\tx\n# comment\n\nT2\ty\nT3#z\n")
    assert salmon_utils.read_targets(p) == ["T9", "T2", "T3"]
    with open(p, "w") as f:
        f.write("T9\tx\n")                                          # (one line: the reference's 0-d array cannot be iterated)
    assert salmon_utils.read_targets(p) == ["T9"]


@pytest.mark.parametrize("name,msg", [("err_no_underscore", "line 4: target name 'T1B'"),
                                      ("err_two_underscores", "line 4: target name 'T1_B_C'"),
                                      ("err_header_dup", "line 5: target name 'T1_A' is listed twice"),
                                      ("err_quant_missing", "target 'T1_B' of the eq_classes header has no line"),
                                      ("err_quant_extra", "line 4: target 'T9_A' is not in the eq_classes header"),
                                      ("dev_quant_dup", "line 4: target 'T1_B' is listed twice")])
def test_host_refusals_of_the_goldens_come_before_the_gpu(golden_dir, tmp_path, name, msg, monkeypatch):
    from alntools_amd import ecb

    def no_gpu(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(ecb, "salmon_ecs", no_gpu)
    out = str(tmp_path / "o.bin")
    with pytest.raises(ValueError, match=msg):
        salmon_utils.convert(os.path.join(golden_dir, "salmon_" + name), out)
    assert not os.path.exists(out)


def test_gz_file_reads_as_the_plain_one(golden_dir, tmp_path):
    src = os.path.join(golden_dir, "salmon_h8")
    d = str(tmp_path / "gz")
    shutil.copytree(src, d)
    plain = os.path.join(d, "aux_info", "eq_classes.txt")
    raw = _bytes(plain)
    with gzip.open(plain + ".gz", "wb") as f:
        f.write(raw)
    assert salmon_utils.eq_classes_path(d) == plain                     # (the plain file wins when both exist)
    os.remove(plain)
    assert salmon_utils.eq_classes_path(d) == plain + ".gz"
    assert salmon_utils.read_eq_classes(plain + ".gz") == raw
    got, exp = chk.expected_from_dir(d), chk.expected_from_dir(src)
    for g, e in zip(got, exp):
        assert np.array_equal(np.asarray(g), np.asarray(e))


def test_writer_round_trips_through_the_checker():
    rng = np.random.default_rng(3)
    ptr, tid, counts = chk.random_ecs(rng, 50, 200)
    rows, cnt = chk.parse_section(chk.ec_section(ptr, tid, counts, crlf=True), 200, 50)
    assert [t for r in rows for t in r] == tid.tolist() and cnt.tolist() == counts.tolist()
    rng = np.random.default_rng(4)
    ptr, tid, counts = chk.random_ecs_fast(rng, 10_000, 2_000)
    rows, cnt = chk.parse_section(chk.ec_section(ptr, tid, counts), 2_000, 10_000)
    assert [t for r in rows for t in r] == tid.tolist()
