"""ecselect without a GPU: the select checker (tests/select_checker.py) pinned to the thresholded ``.bin`` files the reference wrote and to
what its ``get_unique_reads`` returned on every recorded case, every rule on hand-made matrices, and the command's wiring, refusals and
exit status with the device call replaced by the checker."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import select_checker as schk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "select_cases.json")))["cases"]
THRESHOLDED = [("g4_multi_min0.bin", 20, "g4_multi_min20.bin", (21, 20), (8, 5)), ("g4_multi_min0.bin", 60, "g4_multi_min60.bin", (21, 19), (8, 3)),
               ("g4b_multi_min0.bin", 40, "g4b_multi_min40.bin", (845, 821), (338, 80)),
               ("g4b_multi_min0.bin", 160, "g4b_multi_min160.bin", (845, 785), (338, 34)),
               ("g4_multi_min20.bin", 60, "g4_multi_min60.bin", None, None), ("g4_multi_min0.bin", 0, "g4_multi_min0.bin", None, None)]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    """The command sets the package logger's level (``-v``); tests after these ones find it as it was."""
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


# ---- the reference's bytes and pulls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,m,dst,ecs,samples", THRESHOLDED, ids=["%s-m%d" % (t[0][:-4], t[1]) for t in THRESHOLDED])
def test_the_checker_with_a_threshold_gives_the_references_thresholded_file(golden_dir, src, m, dst, ecs, samples):
    a = bin_utils.ecload(os.path.join(golden_dir, src))
    got = schk.select(a, mincount=m)
    assert bin_utils.ecsave2_bytes(got) == _bytes(os.path.join(golden_dir, dst))
    if ecs:
        assert (a.num_reads, got.num_reads) == ecs and (a.num_samples, got.num_samples) == samples


def test_the_recorded_cases_are_the_ones_the_issue_names():
    assert [(c["name"], c["ec"]) for c in CASES] == [("c1", "g2_c1.bin"), ("h8", "gt_h8_in.bin"), ("ms", "g4b_multi_min0.bin"),
                                                     ("c1_gt", "gt_c1.out.bin"), ("ms_gt", "gt_ms.out.bin")]
    assert [(c["rows"]["allele"], c["rows"]["locus"], c["shape"][2]) for c in CASES] == [
        (356, 953, 3313), (10, 278, 3000), (60, 90, 845), (816, 973, 3313), (390, 412, 845)]


def _rows_of(m):
    """{row: [(column, mask), ...]} of the rows of A that hold a mask other than 0."""
    out = {}
    for e in range(m.num_reads):
        r = [(int(c), int(d)) for c, d in zip(m.indicesA[m.indptrA[e]:m.indptrA[e + 1]], m.dataA[m.indptrA[e]:m.indptrA[e + 1]]) if d]
        if r:
            out[e] = r
    return out


@pytest.mark.parametrize("pull,row_class", [("allele", "unique"), ("locus", "locus-unique")])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_checker_put_back_at_the_old_row_numbers_is_the_references_pull(golden_dir, case, pull, row_class):
    m = bin_utils.ecload(os.path.join(golden_dir, case["ec"]))
    T, H, E = case["shape"]
    assert (m.num_loci, m.num_haplotypes, m.num_reads) == (T, H, E)
    z = np.load(os.path.join(golden_dir, case["npz"]))
    ref = {}
    for h in range(H):
        ptr, idx = z[pull + "_indptr"][h], z[pull + "_indices"][z[pull + "_start"][h]:z[pull + "_start"][h + 1]]
        assert len(ptr) == T + 1 and ptr[-1] == len(idx)
        for t in range(T):
            for e in idx[ptr[t]:ptr[t + 1]]:
                ref.setdefault(int(e), {}).setdefault(t, 0)
                ref[int(e)][t] |= 1 << h
    ref = {e: sorted(r.items()) for e, r in ref.items()}
    assert len(ref) == case["rows"][pull]
    out, stay, rows = schk.select_flags(m, row_class)
    old = np.flatnonzero(rows)
    assert stay.all() and out.num_reads == len(old) and out.sname == m.sname
    got = {int(old[e]): r for e, r in _rows_of(out).items()}
    assert got == ref                                   # the kept rows are the reference's, every other row of its result is empty
    assert 0 < len(old) < E
    # the counts: the reference's at the kept rows, nothing elsewhere
    if pull + "_count" in z.files:
        cnt = z[pull + "_count"]
        assert out.num_samples == 1 and np.array_equal(out.indicesN, np.arange(len(old)))
        assert np.array_equal(cnt[old], out.dataN) and cnt.sum() == out.dataN.sum() and np.all(out.dataN > 0)
    else:
        ptr, idx, dat = (z[pull + "_count_" + k] for k in ("indptr", "indices", "data"))
        assert np.array_equal(ptr, out.indptrN) and np.array_equal(idx, old[out.indicesN]) and np.array_equal(dat, out.dataN)


# ---- every rule on hand-made matrices ----------------------------------------------------------------------------------------------------
def _m(rows, counts, H=3, T=6, sname=None):
    """ECMatrices from rows of (columns, masks) and per sample a list of (row, count) entries, in the order given."""
    ip = np.cumsum([0] + [len(r[0]) for r in rows])
    ix = [c for r in rows for c in r[0]]
    dx = [d for r in rows for d in r[1]]
    ipn = np.cumsum([0] + [len(c) for c in counts])
    sname = sname or ["s%d" % s for s in range(len(counts))]
    return bin_utils.ECMatrices(["h%d" % h for h in range(H)], ["t%d" % t for t in range(T)], np.arange(T * H).reshape(T, H) + 100, sname, ip, ix, dx,
                                ipn, [e for c in counts for e, _ in c], [v for c in counts for _, v in c])


BOUNDARY = [((), ()),                   # 0: bits 0, nz 0
            ((2,), (4,)),               # 1: bits 1, nz 1
            ((2,), (5,)),               # 2: one locus with two haplotypes: bits 2, nz 1
            ((1, 4), (1, 2)),           # 3: bits 2, nz 2
            ((0, 3), (0, 2)),           # 4: a stored 0 beside one real non-zero: bits 1, nz 1
            ((0,), (0,)),               # 5: a stored 0 alone: bits 0, nz 0
            ((0, 1, 5), (1, 0, 6))]     # 6: bits 3, nz 2


def test_the_class_boundaries():
    m = _m(BOUNDARY, [[(e, e + 1) for e in range(7)]])
    bits, nz = schk.row_counts(m)
    assert bits.tolist() == [0, 1, 2, 2, 1, 0, 3] and nz.tolist() == [0, 1, 1, 2, 1, 0, 2]
    assert np.flatnonzero(schk.in_class(m, None)).tolist() == [0, 1, 2, 3, 4, 5, 6]         # empty rows included
    assert np.flatnonzero(schk.in_class(m, "unique")).tolist() == [1, 4]
    assert np.flatnonzero(schk.in_class(m, "locus-unique")).tolist() == [1, 2, 4]
    assert np.flatnonzero(schk.in_class(m, "multi")).tolist() == [3, 6]
    u = schk.select(m, "unique")
    assert u.indptrA.tolist() == [0, 1, 3] and u.indicesA.tolist() == [2, 0, 3] and u.dataA.tolist() == [4, 0, 2]       # the stored 0 is copied
    assert u.indptrN.tolist() == [0, 2] and u.indicesN.tolist() == [0, 1] and u.dataN.tolist() == [2, 5]
    a = schk.select(m)
    assert bin_utils.ecsave2_bytes(a) == bin_utils.ecsave2_bytes(m)
    lu = schk.select(m, "locus-unique")
    assert lu.indptrA.tolist() == [0, 1, 2, 4] and lu.dataN.tolist() == [2, 3, 5]
    mu = schk.select(m, "multi")
    assert mu.indptrA.tolist() == [0, 2, 5] and mu.indicesA.tolist() == [1, 4, 0, 1, 5] and mu.dataN.tolist() == [4, 7]
    assert mu.lname == m.lname and mu.hname == m.hname and np.array_equal(mu.lengths, m.lengths)


def test_the_totals_are_taken_after_the_class_and_the_threshold_sits_on_the_total():
    # sample s0 counts 10 in unique rows and 90 elsewhere, s1 counts 30 in unique rows only
    m = _m(BOUNDARY, [[(1, 4), (3, 90), (4, 6)], [(1, 30)]])
    assert schk.select(m, None, mincount=31).sname == ["s0"]
    assert schk.select(m, "unique", mincount=11).sname == ["s1"]
    for n, names in ((9, ["s0", "s1"]), (10, ["s0", "s1"]), (11, ["s1"]), (29, ["s1"]), (30, ["s1"]), (31, [])):
        assert schk.select(m, "unique", mincount=n).sname == names, n
    one = bin_utils.ecsave2_bytes(schk.select(m, "unique", mincount=1))
    assert bin_utils.ecsave2_bytes(schk.select(m, "unique", mincount=0)) == one
    assert bin_utils.ecsave2_bytes(schk.select(m, "unique", mincount=-3)) == one


def test_a_named_sample_without_a_read_stays_without_a_threshold_and_leaves_with_one():
    m = _m(BOUNDARY, [[(1, 4)], [(3, 9)], [(4, 0)], []])
    u = schk.select(m, "unique")
    assert u.sname == ["s0", "s1", "s2", "s3"] and u.indptrN.tolist() == [0, 1, 1, 1, 1] and u.num_reads == 1
    assert schk.select(m, "unique", mincount=0).sname == ["s0"]
    assert schk.select(m, "unique", samples=["s3", "s1"]).sname == ["s1", "s3"]
    assert schk.select(m, "unique", samples=["s3", "s1"]).num_reads == 0


def test_duplicates_are_copied_zero_counts_dropped_and_the_order_of_the_samples_is_the_files():
    m = _m(BOUNDARY, [[(3, 5), (1, 2), (1, 3), (6, 0), (4, 1)], [(6, 7)], [(0, 1), (5, 2)]], sname=["a", "b", "c"])
    out = schk.select(m, samples=["c", "a", "c"])
    assert out.sname == ["a", "c"]
    # rows 0, 1, 3, 4, 5 stay (6 is counted 0 by a and only by b otherwise); an EC listed twice stays listed twice, in the input's order
    assert out.indptrN.tolist() == [0, 4, 6] and out.indicesN.tolist() == [2, 1, 1, 3, 0, 4] and out.dataN.tolist() == [5, 2, 3, 1, 1, 2]
    assert out.indptrA.tolist() == [0, 0, 1, 3, 5, 6]
    with pytest.raises(KeyError, match="nope"):
        schk.select(m, samples=["a", "nope"])


def test_a_row_in_class_that_nobody_counts_leaves_the_file_though_the_reference_keeps_it():
    """The deviation: ``pull_alignments_from`` keeps every row and empties the ones not chosen, so a uniquely aligning row with count 0 is
    still a row of its result; here rows that keep no count leave the file."""
    m = _m(BOUNDARY, [[(1, 0), (4, 3)]])
    out, stay, rows = schk.select_flags(m, "unique")
    assert schk.in_class(m, "unique")[1] and not rows[1] and rows.tolist() == [False] * 4 + [True] + [False] * 2
    assert out.num_reads == 1 and out.indicesA.tolist() == [0, 3] and out.dataN.tolist() == [3]


# ---- bin_utils and the command line, the checker in the device's place -------------------------------------------------------------------
def _fake_select(indptrA, indicesA, dataA, indptrN, indicesN, dataN, n_loci, n_haps, row_class=None, sample_keep=None, min_count=None, device=0):
    m = bin_utils.ECMatrices(["h"] * n_haps, ["t%d" % t for t in range(n_loci)], np.zeros((n_loci, n_haps)), ["s%d" % s for s in range(len(indptrN) - 1)],
                             indptrA, indicesA, dataA, indptrN, indicesN, dataN)
    o, stay, _ = schk.select_flags(m, row_class, sample_keep, min_count)
    return (o.indptrA, o.indicesA, o.dataA, o.indptrN, o.indicesN, o.dataN), stay


def test_ecselect_with_the_checker_as_the_device_writes_the_references_bytes(golden_dir, tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "select", _fake_select)
    out = str(tmp_path / "o.bin")
    with caplog.at_level("INFO", logger="alntools.utils"):
        bin_utils.ecselect(os.path.join(golden_dir, "g4b_multi_min0.bin"), out, mincount=160)
    assert _bytes(out) == _bytes(os.path.join(golden_dir, "g4b_multi_min160.bin"))
    assert "ECs: 785 (from 845 rows)" in caplog.text and "samples: 34 (from 338)" in caplog.text
    os.remove(out)
    src = os.path.join(golden_dir, "g4_multi_min0.bin")
    m = bin_utils.ecload(src)
    names = tmp_path / "names.txt"
    names.write_text("\n%s\n\n  %s  \n%s\n" % (m.sname[5], m.sname[2], m.sname[5]))
    bin_utils.ecselect(src, out, row_class="multi", samples=[m.sname[7]], samples_file=str(names))
    assert _bytes(out) == schk.select_bytes(m, "multi", [m.sname[2], m.sname[5], m.sname[7]])
    assert bin_utils.ecload(out).sname == [m.sname[2], m.sname[5], m.sname[7]]
    os.remove(out)
    for kw, text in ((dict(mincount=10 ** 9), "no sample left"), (dict(samples=[m.sname[0]], row_class="unique", mincount=None), None),
                     (dict(samples=["nobody"]), "nobody"), (dict(row_class="best"), "no such read class")):
        if text is None:                                                    # a sample without a uniquely aligning read: found on the fixture
            u = schk.select_flags(m, "unique")[0]
            empty = [s for k, s in enumerate(u.sname) if u.indptrN[k] == u.indptrN[k + 1]]
            if not empty:
                continue
            kw, text = dict(samples=empty[:1], row_class="unique"), "no read left"
        with pytest.raises((ValueError, KeyError), match=text):
            bin_utils.ecselect(src, out, **kw)
        assert not os.path.exists(out)


def test_no_read_left_is_refused_by_name(tmp_path, monkeypatch):
    monkeypatch.setattr(ecb, "select", _fake_select)
    src, out = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    bin_utils.ecsave2(src, _m(BOUNDARY, [[(3, 5)], [(1, 2)]]))
    with pytest.raises(ValueError, match="no read left"):
        bin_utils.ecselect(src, out, row_class="unique", samples=["s0"])
    with pytest.raises(ValueError, match="no sample left"):
        bin_utils.ecselect(src, out, row_class="unique", samples=["s0"], mincount=1)
    assert not os.path.exists(out)
    bin_utils.ecselect(src, out, row_class="unique")
    assert bin_utils.ecload(out).sname == ["s0", "s1"] and bin_utils.ecload(out).num_reads == 1


def test_the_command_line_hands_its_options_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e, names = tmp_path / "e.bin", tmp_path / "n.txt"
    e.write_bytes(b""); names.write_text("")
    o = str(tmp_path / "o.bin")
    seen = []
    monkeypatch.setattr(methods, "ecselect", lambda *a: seen.append(a))
    r = CliRunner().invoke(cli.cli, ["ecselect", str(e), o, "--locus-unique", "-s", "a", "-s", "b", "--samples", str(names), "-m", "7", "-v"])
    assert r.exit_code == 0, r.output
    r = CliRunner().invoke(cli.cli, ["ecselect", str(e), o])
    assert r.exit_code == 0, r.output
    assert seen == [(str(e), o, "locus-unique", ["a", "b"], str(names), 7), (str(e), o, None, None, None, None)]
    for two in (["--unique", "--multi"], ["--unique", "--locus-unique"], ["--multi", "--locus-unique"]):
        r = CliRunner().invoke(cli.cli, ["ecselect", str(e), o] + two)
        assert r.exit_code == 2 and "at most one of" in r.output and len(seen) == 2

    def boom(*a):
        raise ValueError("no")
    monkeypatch.setattr(methods, "ecselect", boom)
    assert CliRunner().invoke(cli.cli, ["ecselect", str(e), o]).exit_code == 1


# the command in a process of its own, the checker in the device's place
_RUN = """
import sys
sys.path[:0] = [%r, %r]
import test_ecselect
from alntools_amd import ecb, cli
ecb.select = test_ecselect._fake_select
cli.cli()
"""


@pytest.mark.parametrize("what", ["two_classes", "unknown_sample", "unknown_sample_in_file", "no_sample_left", "no_read_left", "not_a_bin", "works"])
def test_command_line_refusals_exit_1_and_write_nothing(golden_dir, tmp_path, what):
    out, src = str(tmp_path / "out.bin"), os.path.join(golden_dir, "g4_multi_min0.bin")
    names = tmp_path / "names.txt"
    m = bin_utils.ecload(src)
    names.write_text("%s\n\nCELL_NOPE\n" % m.sname[0] if what == "unknown_sample_in_file" else "%s\n\n%s\n\n" % (m.sname[3], m.sname[1]))
    args = {"two_classes": ["--unique", "--multi"], "unknown_sample": ["-s", m.sname[0], "-s", "CELL_NOPE"], "unknown_sample_in_file": ["--samples", str(names)],
            "no_sample_left": ["-m", "1000000"], "no_read_left": ["--unique", "-s", "s0"], "not_a_bin": [], "works": ["--samples", str(names), "-m", "1"]}[what]
    if what == "no_read_left":
        src = str(tmp_path / "i.bin")
        bin_utils.ecsave2(src, _m(BOUNDARY, [[(3, 5)], [(1, 2)]]))
    if what == "not_a_bin":
        src = os.path.join(golden_dir, "g2_c1.range.txt")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    r = subprocess.run([sys.executable, "-c", _RUN % (ROOT, os.path.join(ROOT, "tests")), "ecselect", src, out] + args + ["-v"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    if what == "works":
        assert r.returncode == 0, r.stderr
        assert _bytes(out) == schk.select_bytes(m, None, [m.sname[1], m.sname[3]], 1)
        assert "samples: 2 (from 8)" in r.stderr
        return
    assert r.returncode == (2 if what == "two_classes" else 1), r.stdout + r.stderr
    assert not os.path.exists(out)
    if what == "two_classes":
        assert "at most one of" in r.stderr
        return
    assert "Error:" in r.stderr and "libecb" not in r.stderr, r.stderr
    text = {"unknown_sample": "CELL_NOPE", "unknown_sample_in_file": "CELL_NOPE", "no_sample_left": "no sample left", "no_read_left": "no read left"}.get(what)
    assert text is None or text in r.stderr


def test_the_one_gpu_command_imports_no_pytorch():
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    code = "import sys; from alntools_amd import cli, bin_utils; assert hasattr(cli, 'ecselect') and hasattr(bin_utils, 'ecselect'); print('torch' in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr


def test_the_abi_declares_the_select_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_select.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.SELECT_SYMBOLS)
    assert len(re.findall(r'^#\s*include "ecb_select\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.SELECT_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS) | set(ecb.BUNDLE_SYMBOLS))
    assert "ecb_select" not in main.replace('"ecb_select.h"', "")
    from alntools_amd import build
    assert any(p.endswith("ecb_select.h") for p in build.inputs())
    # a C compiler sees them through ecb.h alone
    src = '#include "ecb.h"\nvoid* a = (void*)ecb_select; void* b = (void*)ecb_select_device;\n'
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
