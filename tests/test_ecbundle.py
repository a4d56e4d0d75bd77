"""ecbundle without a GPU: the bundle checker (tests/bundle_checker.py) pinned to what the reference's ``bundle(reset=True)`` returned on
every recorded case, its collapse to the merge checker, ``bin_utils.group_map`` on the fixture group files, the max-length rule, and the
command's wiring and exit status with the device call replaced by the checker."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import bundle_checker as bchk
import ec_merge_checker as chk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "bundle_cases.json")))["cases"]
RECORDED = [c for c in CASES if c["raises"] is None]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _load(golden_dir, case):
    m = bin_utils.ecload(os.path.join(golden_dir, case["ec"]))
    gname, groups = bin_utils.load_groups(m, os.path.join(golden_dir, case["grp"]))
    return m, gname, groups


def test_the_recorded_cases_are_the_ones_the_issue_names():
    assert [(c["name"], c["ec"], c["grp"]) for c in CASES] == [
        ("c1", "g2_c1.bin", "gt_c1.grp.txt"), ("h8", "gt_h8_in.bin", "gt_h8.grp.txt"), ("ms", "g4b_multi_min0.bin", "gt_ms.grp.txt"),
        ("c1_mixed", "g2_c1.bin", "bundle_c1_mixed.grp.txt"), ("err_tx", "g2_c1.bin", "gt_err_tx.grp.txt")]
    assert [c["raises"] for c in CASES] == [None, None, None, None, "KeyError"]


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_the_checkers_uncollapsed_matrix_is_the_references(golden_dir, case):
    """A = sum_h 2^h M_h of the reference's per-haplotype E x G matrices, exactly: same rows, columns ascending, same masks."""
    m, gname, groups = _load(golden_dir, case)
    u = bchk.uncollapsed(m, gname, groups)
    G, H, E = case["shape"]
    assert (u.num_loci, u.num_haplotypes, u.num_reads) == (G, H, E)
    z = np.load(os.path.join(golden_dir, case["npz"]))
    masks = {}
    for h in range(H):
        ptr, idx = z["indptr"][h], z["indices"][z["start"][h]:z["start"][h + 1]]
        assert len(ptr) == G + 1 and ptr[-1] == len(idx)
        for g in range(G):
            for e in idx[ptr[g]:ptr[g + 1]]:
                masks[(int(e), g)] = masks.get((int(e), g), 0) | (1 << h)
    ref = sorted(masks.items())
    got = [((e, int(u.indicesA[q])), int(u.dataA[q])) for e in range(E) for q in range(int(u.indptrA[e]), int(u.indptrA[e + 1]))]
    assert got == ref
    assert list(u.lname) == list(gname) and u.sname == m.sname and u.hname == m.hname
    assert np.array_equal(u.indptrN, m.indptrN) and np.array_equal(u.indicesN, m.indicesN) and np.array_equal(u.dataN, m.dataN)


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_the_collapsed_output_is_the_merge_of_the_uncollapsed(golden_dir, case):
    m, gname, groups = _load(golden_dir, case)
    u = bchk.uncollapsed(m, gname, groups)
    assert bchk.bundle_bytes(m, gname, groups) == chk.merge_bytes([u])
    b = bchk.bundle(m, gname, groups)
    assert b.num_reads < m.num_reads                      # isoform-level ECs fold into gene-level ones
    rows = set()
    for e in range(b.num_reads):
        key = tuple(zip(b.indicesA[b.indptrA[e]:b.indptrA[e + 1]].tolist(), b.dataA[b.indptrA[e]:b.indptrA[e + 1]].tolist()))
        assert key not in rows and list(key) == sorted(key)
        rows.add(key)
    assert int(b.dataN.sum()) == int(m.dataN.sum())      # counts >= 0: no sum becomes 0, nothing is dropped


def test_the_group_without_a_transcript_is_an_empty_column_in_the_reference_too(golden_dir):
    case = next(c for c in CASES if c["name"] == "c1_mixed")
    m, gname, groups = _load(golden_dir, case)
    assert groups[17] == [] and gname[17] == "M00017"
    z = np.load(os.path.join(golden_dir, case["npz"]))
    assert all(z["indptr"][h][17] == z["indptr"][h][18] for h in range(2))
    u = bchk.uncollapsed(m, gname, groups)
    assert 17 not in set(u.indicesA.tolist()) and len(u.lname) == 60
    assert any(len(t) != len(set(t)) for t in groups)                     # a transcript repeated on one line
    flat = [t for tids in groups for t in set(tids)]
    assert len(flat) != len(set(flat)) and len(set(flat)) < m.num_loci    # one in two groups, some in none


def test_group_map_on_the_fixture_files(golden_dir):
    for case in RECORDED:
        m, gname, groups = _load(golden_dir, case)
        if case["name"] == "c1":                                          # (G00003 is on two lines of gt_c1.grp.txt)
            with pytest.raises(ValueError, match="G00003"):
                bin_utils.group_map(m, os.path.join(golden_dir, case["grp"]))
            continue
        names, ptr, idx, lengths = bin_utils.group_map(m, os.path.join(golden_dir, case["grp"]))
        eptr, eidx = bchk.group_csr(m.num_loci, groups)
        assert names == gname and len(ptr) == m.num_loci + 1
        assert np.array_equal(ptr, eptr) and np.array_equal(idx, eidx)
        assert np.array_equal(lengths, bchk.group_lengths(m, groups))
        for t in range(m.num_loci):
            assert np.all(np.diff(idx[ptr[t]:ptr[t + 1]]) > 0)
    m = bin_utils.ecload(os.path.join(golden_dir, "g2_c1.bin"))
    with pytest.raises(KeyError, match="TX_NOPE"):
        bin_utils.group_map(m, os.path.join(golden_dir, "gt_err_tx.grp.txt"))


def _small():
    lens = np.array([[10, 20], [30, 5], [7, 7], [1, 99]])
    return bin_utils.ECMatrices(["A", "B"], ["t0", "t1", "t2", "t3"], lens, ["s", "u"], [0, 2, 3, 3, 5, 6], [0, 1, 1, 0, 3, 2],
                                [1, 2, 2, 1, 3, 1], [0, 3, 5], [0, 1, 3, 1, 4], [4, 5, 6, 7, 8])


def _grp(tmp_path, lines, name="g.txt"):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write("".join("\t".join(ln) + "\n" for ln in lines))
    return p


def test_the_length_of_a_group_is_its_longest_member_per_haplotype(tmp_path):
    """A deviation from the reference, which leaves ``lengths`` at transcript shape (its ecsave2 could not write G targets with them)."""
    m = _small()
    grp = _grp(tmp_path, [["g0", "t0", "t1"], ["g1"], ["g2", "t3", "t3", "t1"]])
    names, ptr, idx, lengths = bin_utils.group_map(m, grp)
    assert names == ["g0", "g1", "g2"]
    assert lengths.tolist() == [[30, 20], [0, 0], [30, 99]]
    assert ptr.tolist() == [0, 1, 3, 3, 4] and idx.tolist() == [0, 0, 2, 2]
    b = bchk.bundle(m, *bin_utils.load_groups(m, grp))
    assert np.array_equal(b.lengths, lengths)
    # rows 2 (empty) and 4 (its only transcript is in no group) share the empty key
    assert b.indptrA.tolist() == [0, 2, 4, 4, 6] and b.indicesA.tolist() == [0, 2, 0, 2, 0, 2] and b.dataA.tolist() == [3, 2, 2, 2, 1, 3]
    assert b.indptrN.tolist() == [0, 3, 5] and b.indicesN.tolist() == [0, 1, 3, 1, 2] and b.dataN.tolist() == [4, 5, 6, 7, 8]


def test_a_group_name_on_two_lines_is_refused_with_its_name(tmp_path):
    with pytest.raises(ValueError, match="gX is listed more than once"):
        bin_utils.group_map(_small(), _grp(tmp_path, [["gX", "t0"], ["gY", "t1"], ["gX", "t2"]]))


def _fake_bundle(indptrA, indicesA, dataA, indptrN, indicesN, dataN, n_loci, n_haps, n_groups, map_ptr, map_idx, device=0):
    """ecb.bundle through the checker: the map read back into per-group member lists."""
    groups = [[] for _ in range(n_groups)]
    for t in range(n_loci):
        for g in map_idx[map_ptr[t]:map_ptr[t + 1]]:
            groups[int(g)].append(t)
    m = bin_utils.ECMatrices(["h"] * n_haps, ["t%d" % t for t in range(n_loci)], np.zeros((n_loci, n_haps)), ["s%d" % s for s in range(len(indptrN) - 1)],
                             indptrA, indicesA, dataA, indptrN, indicesN, dataN)
    b = bchk.bundle(m, ["g%d" % g for g in range(n_groups)], groups)
    return b.indptrA, b.indicesA, b.dataA, b.indptrN, b.indicesN, b.dataN


def test_ecbundle_with_the_checker_as_the_device_writes_the_checkers_bytes(golden_dir, tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "bundle", _fake_bundle)
    out = str(tmp_path / "o.bin")
    for case in RECORDED:
        if case["name"] == "c1":
            continue
        m, gname, groups = _load(golden_dir, case)
        with caplog.at_level("INFO"):
            bin_utils.ecbundle(os.path.join(golden_dir, case["ec"]), os.path.join(golden_dir, case["grp"]), out)
        exp = bchk.bundle(m, gname, groups)
        assert _bytes(out) == bin_utils.ecsave2_bytes(exp)
        assert "Number of equivalence classes: {:,} (from {:,} rows)".format(exp.num_reads, m.num_reads) in caplog.text
        os.remove(out)


def test_the_command_line_hands_its_three_files_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e, g = tmp_path / "e.bin", tmp_path / "g.txt"
    e.write_bytes(b""); g.write_text("")
    seen = []
    monkeypatch.setattr(methods, "ecbundle", lambda *a: seen.append(a))
    r = CliRunner().invoke(cli.cli, ["ecbundle", str(e), str(g), str(tmp_path / "o.bin"), "-v"])
    assert r.exit_code == 0, r.output
    assert seen == [(str(e), str(g), str(tmp_path / "o.bin"))]

    def boom(*a):
        raise ValueError("no")
    monkeypatch.setattr(methods, "ecbundle", boom)
    assert CliRunner().invoke(cli.cli, ["ecbundle", str(e), str(g), str(tmp_path / "o.bin")]).exit_code == 1


@pytest.mark.parametrize("what", ["duplicate_group", "unknown_transcript", "no_groups", "not_a_bin"])
def test_command_line_refusals_exit_1_and_write_nothing(golden_dir, tmp_path, what):
    """Every host-side refusal ends the command before libecb is loaded."""
    out = str(tmp_path / "out.bin")
    ec = os.path.join(golden_dir, "g2_c1.bin")
    grp = {"duplicate_group": os.path.join(golden_dir, "gt_c1.grp.txt"), "unknown_transcript": os.path.join(golden_dir, "gt_err_tx.grp.txt"),
           "no_groups": _grp(tmp_path, []), "not_a_bin": os.path.join(golden_dir, "bundle_c1_mixed.grp.txt")}[what]
    if what == "not_a_bin":
        ec = os.path.join(golden_dir, "g2_c1.range.txt")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecbundle", ec, grp, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Error:" in r.stderr and "libecb" not in r.stderr, r.stderr
    if what == "duplicate_group":
        assert "G00003" in r.stderr
    if what == "unknown_transcript":
        assert "TX_NOPE" in r.stderr
    assert not os.path.exists(out)


def test_the_abi_declares_the_bundle_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_bundle.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    import re
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.BUNDLE_SYMBOLS)
    assert len(re.findall(r'^#\s*include "ecb_bundle\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.BUNDLE_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS))
    assert "ecb_bundle" not in main.replace('"ecb_bundle.h"', "")
    # a C compiler sees them through ecb.h alone
    src = '#include "ecb.h"\nvoid* a = (void*)ecb_bundle; void* b = (void*)ecb_bundle_device;\n'
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
