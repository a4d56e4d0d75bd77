"""ecquant per cell without a GPU: the cell checker (tests/cell_quant_checker.py) pinned to the step pairs recorded from the reference -- cell 0
of ``g4b_multi_min0.bin`` (``quant_ms_s0.npz``) and four more of its cells (``quant_cells_cases.json``) --, the constants the GPU tests place
their shapes on, the ABI's header, the command's wiring, its tables and the host's refusals.

The tolerance of one step of one cell is ``test_ecquant.py``'s, with the cell's own B and L: (B + L + 4) 2^-52 relative, entry by entry, the
same entries 0."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import cell_quant_checker as cq
import counts_checker
import quant_checker as qchk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "alntools_amd", "csrc", "quant_cells.inc")
MS = os.path.join(GOLDEN, "g4b_multi_min0.bin")
CELL_CASES = json.load(open(os.path.join(GOLDEN, "quant_cells_cases.json")))["cases"]
#: every recorded (cell, k) -> (the .npz, the prefix of its arrays)
RECORDED = [(0, k, "quant_ms_s0.npz", "") for k in (0, 1, 5, 20)] + [(c["cell"], k, c["npz"], c["prefix"]) for c in CELL_CASES for k in c["steps"]]
QC_LONG_ROW, QC_LONG_COL, QC_TILE, TPB = 256, 32, 2048, 256          # what the GPU tests import
PINNED = [
    ("QC_LONG_ROW", "256", "test_edges (an entry whose row has more non-zeros is summed by a workgroup)"),
    ("QC_LONG_COL", "32", "test_edges (a slot with more column entries is summed by a workgroup of its own)"),
    ("QC_TILE", "2048", "test_many_workgroups (expanded non-zeros a workgroup stages at a time)"),
]
_loaded = {}


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


def ms():
    """(ECMatrices of g4b_multi_min0.bin, its cells), loaded once."""
    if "ms" not in _loaded:
        m = bin_utils.ecload(MS)
        _loaded["ms"] = (m, cq.cells(m))
    return _loaded["ms"]


def npz(name):
    if name not in _loaded:
        _loaded[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _loaded[name]


# ---- the checker against the reference ----------------------------------------------------------------------------------------------------
def test_the_recorded_cells_are_the_ones_the_issue_names():
    m, cs = ms()
    entries = np.array([len(c.rows) for c in cs])
    assert m.num_samples == 338 and [c["steps"] for c in CELL_CASES] == [[0, 1, 5]] * 4
    most, single = CELL_CASES[0], CELL_CASES[1]
    assert most["cell"] == int(np.argmax(entries)) and most["entries"] == entries.max() == 296
    assert single["entries"] == 1 and entries[single["cell"]] == 1
    assert len({c["cell"] for c in CELL_CASES} | {0}) == 5
    assert os.path.getsize(os.path.join(GOLDEN, "quant_cells.npz")) <= 970265
    for case in CELL_CASES:
        cell, z = cs[case["cell"]], npz(case["npz"])
        assert len(cell.rows) == case["entries"] and (cell.p.B, cell.p.L) == (case["B"], case["L"])
        w = counts_checker.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN, case["cell"])
        assert np.array_equal(w, z[case["prefix"] + "w"])
        assert np.array_equal(cell.p.aln(), z[case["prefix"] + "theta_0"])          # theta_0 is the cell's aln, exactly
        assert np.array_equal(cell.support, np.flatnonzero(z[case["prefix"] + "theta_0"].sum(axis=0) > 0))


@pytest.mark.parametrize("c,k,file,pre", RECORDED, ids=["cell%d-k%d" % r[:2] for r in RECORDED])
def test_the_cell_checkers_step_reproduces_every_recorded_pair(c, k, file, pre):
    cell, z = ms()[1][c], npz(file)
    got, explained = cell.step(z[pre + "theta_%d" % k])
    worst = qchk.agree(got, z[pre + "next_%d" % k], cell.tolerance())
    print("cell %d k=%d: worst relative difference %.3g, bound %.3g" % (c, k, worst, cell.tolerance()))
    assert explained == cell.W == int(z[pre + "w"].sum()) if pre else explained == cell.W
    assert not got[:, np.setdiff1d(np.arange(cell.p.T), cell.support)].any()


def test_a_cells_rows_support_w_and_the_twice_listed_ec():
    # rows of A: 0 -> (t0: h0), 1 -> (t1: h0 h1, t3: h1), 2 -> (t2: stored 0), 3 -> (t0: h1, t1: h0)
    A = ([0, 1, 3, 4, 6], [0, 1, 3, 2, 0, 1], [1, 3, 2, 0, 2, 1], 4, 2)
    # cells: 0 lists EC 1 twice and EC 3; 1 is empty; 2 has counts of 0 only; 3 has only the row of stored zeros; 4 lists EC 0 and a zero count
    N = ([0, 3, 3, 5, 6, 8], [1, 3, 1, 0, 1, 2, 0, 3], [4, 2, 6, 0, 0, 9, 5, 0])
    cs = [cq.Cell(*(A + N + (c,))) for c in range(5)]
    assert [len(c.rows) for c in cs] == [3, 0, 0, 1, 1] and [c.support.tolist() for c in cs] == [[0, 1, 3], [], [], [], [0]]
    assert [c.W for c in cs] == [12, 0, 0, 0, 5] and (cs[0].p.B, cs[0].p.L) == (3, 3)
    assert cs[0].p.aln().tolist() == [[0.0, 12.0, 0.0, 0.0], [2.0, 10.0, 0.0, 10.0]]
    # two rows of 4 and 6 reads are one row of 10, up to rounding
    one = cq.Cell(*(A + ([0, 2], [1, 3], [10, 2]) + (0,)))
    a, ea = cs[0].step(cs[0].p.aln())
    b, eb = one.step(one.p.aln())
    assert ea == eb == 12 and np.allclose(a, b, rtol=1e-15, atol=0)
    ptr, loc, theta, info = cq.quantify_cells(*(A + N), max_iters=0)
    assert ptr.tolist() == [0, 3, 3, 3, 3, 4] and loc.tolist() == [0, 1, 3, 0] and theta.tolist() == [[0, 2], [12, 10], [0, 10], [5, 0]]
    assert info["converged"].all() and not info["n_iter"].any()
    ptr, loc, theta, info = cq.quantify_cells(*(A + N), cell_keep=[1, 0, 1, 1, 0], tol=0.0, max_iters=3)
    assert ptr.tolist() == [0, 3, 3, 3, 3, 3] and info["n_iter"].tolist() == [3, 0, 0, 0, 0] and info["converged"].tolist() == [False] + [True] * 4


# ---- the constants and the ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value,test", PINNED, ids=[p[0] for p in PINNED])
def test_constants_the_cell_tests_straddle(name, value, test):
    defs = re.findall(r"constexpr\s+u32\s+%s\s*=\s*([^;,]+);" % name, open(SRC).read())
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecquant_cells.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


def test_the_thresholds_are_the_ones_the_kernels_branch_on_and_no_sum_is_a_float_atomic():
    src = open(SRC).read()
    assert len(re.findall(r"b - a <= QC_LONG_ROW", src)) == 1 and len(re.findall(r"n > QC_LONG_ROW", src)) == 1
    assert len(re.findall(r"> QC_LONG_COL", src)) == 2                  # k_qc_cols lists the long columns, k_qc_mstep takes their sums
    assert "atomicAdd(reinterpret_cast<double" not in src and "unsafeAtomicAdd" not in src and "atomicAdd(&d" not in src
    assert (QC_LONG_ROW, QC_LONG_COL, QC_TILE) == (256, 32, 2048)
    main = open(os.path.join(ROOT, "alntools_amd", "csrc", "ecb.hip")).read()
    assert int(re.search(r"constexpr int TPB = (\d+);", main).group(1)) == TPB
    assert len(re.findall(r'^#include "quant_cells\.inc"', main, re.M)) == 1


def test_the_abi_declares_the_cell_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_quant_cells.h")).read()
    quant = open(os.path.join(ROOT, "include", "ecb_quant.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert ecb.QUANT_CELLS_SYMBOLS == ("ecb_cell_support_device", "ecb_cell_support", "ecb_quantify_cells_device", "ecb_quantify_cells")
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.QUANT_CELLS_SYMBOLS)
    assert len(re.findall(r'^#include "ecb_quant_cells\.h"', quant, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.QUANT_CELLS_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS) | set(ecb.BUNDLE_SYMBOLS) | set(ecb.SELECT_SYMBOLS)
                                               | set(ecb.QUANT_SYMBOLS) | set(ecb.QUANT_MODEL_SYMBOLS))
    from alntools_amd import build
    assert any(p.endswith("ecb_quant_cells.h") for p in build.inputs()) and any(p.endswith("quant_cells.inc") for p in build.inputs())
    src = ('#include "ecb.h"\nvoid* a = (void*)ecb_cell_support; void* b = (void*)ecb_cell_support_device;\n'
           "void* c = (void*)ecb_quantify_cells; void* d = (void*)ecb_quantify_cells_device;\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the command, its tables and the host's refusals --------------------------------------------------------------------------------------
def test_the_command_line_hands_its_options_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e = tmp_path / "e.bin"
    e.write_bytes(b"")
    names = tmp_path / "names.txt"
    names.write_text("a\n")
    o, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    seen = []
    monkeypatch.setattr(methods, "ecquant_cells", lambda *a: seen.append(a))
    r = CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o, "-s", "c1", "-s", "c2", "--samples", str(names), "-l", "-i", "25", "-t", "1e-3",
                                     "--report", rep, "-v"])
    assert r.exit_code == 0, r.output
    r = CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o])
    assert r.exit_code == 0, r.output
    assert seen == [(str(e), o, ["c1", "c2"], str(names), True, 25, 1e-3, rep), (str(e), o, None, None, False, 1000, 1e-6, None)]
    assert CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o, "-i", "-1"]).exit_code == 2 and len(seen) == 2

    def boom(*a):
        raise ValueError("no")
    monkeypatch.setattr(methods, "ecquant_cells", boom)
    assert CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o]).exit_code == 1
    assert "``ecquant-cells``" in cli.__doc__


def test_the_tables_and_their_numbers_read_back_exactly():
    theta = np.array([[1.5, 2.0], [0.0, 1e-30], [1.0 / 3.0, 7.0]])
    text = bin_utils.cells_table(["s0", "s1", "s2"], ["tA", "tB", "tC"], ["P", "M"], [0, 2, 2, 3], [0, 2, 1], theta)
    assert text == ("sample\tlocus\tP\tM\ttotal\n" "s0\ttA\t1.5\t2.0\t3.5\n" "s0\ttC\t0.0\t1e-30\t1e-30\n"
                    "s2\ttB\t0.3333333333333333\t7.0\t7.333333333333333\n")
    back = np.array([[float(v) for v in ln.split("\t")[2:4]] for ln in text.splitlines()[1:]])
    assert back.tobytes() == theta.tobytes()
    info = {"n_iter": np.array([3, 0, 1000], dtype=np.uint32), "delta": np.array([1e-7, 0.0, 2.5]), "explained": np.array([12, 0, 7]),
            "converged": np.array([True, True, False])}
    assert bin_utils.cells_report(["s0", "s1", "s2"], info) == ("sample\tn_iter\tdelta\texplained\tconverged\n" "s0\t3\t1e-07\t12\t1\n"
                                                                 "s1\t0\t0.0\t0\t1\n" "s2\t1000\t2.5\t7\t0\n")
    assert bin_utils.cells_report(["s0", "s1", "s2"], info, [False, False, True]).splitlines()[1:] == ["s2\t1000\t2.5\t7\t0"]


def _fake_count(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, device=0):
    return counts_checker.count(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample)


def test_ecquant_cells_with_the_checker_as_the_device_writes_the_checkers_tables(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "quantify_cells", cq.quantify_cells, raising=False)
    monkeypatch.setattr(ecb, "count_alignments", _fake_count)
    m, cs = ms()
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    names = [m.sname[3], m.sname[157]]
    keep = np.isin(np.arange(m.num_samples), [3, 157])
    with caplog.at_level("INFO", logger="alntools.utils"):
        bin_utils.ecquant_cells(MS, out, samples=names, max_iters=9, tol=0.0, report=rep)
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    ptr, loc, theta, info = cq.quantify_cells(*a, cell_keep=keep, max_iters=9, tol=0.0)
    assert open(out).read() == bin_utils.cells_table(m.sname, m.lname, m.hname, ptr, loc, theta)
    assert open(rep).read() == bin_utils.cells_report(m.sname, info, keep) and len(open(rep).read().splitlines()) == 3
    assert "Estimating abundances of 2 cells" in caplog.text and "cells not converged: 1" in caplog.text      # (the single entry of cell 157: delta 0 at once)
    os.remove(out)
    # -l: scale = 1 / length, refused by name where the pooled file has alignments and no length
    bin_utils.ecquant_cells(MS, out, samples=names, use_lengths=True, max_iters=4, tol=0.0)
    ptr, loc, theta, info = cq.quantify_cells(*a, cell_keep=keep, scale=1.0 / np.asarray(m.lengths).T, max_iters=4, tol=0.0)
    assert open(out).read() == bin_utils.cells_table(m.sname, m.lname, m.hname, ptr, loc, theta)


def test_the_host_refuses_an_unknown_sample_and_a_length_of_zero_under_l_by_name(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "quantify_cells", cq.quantify_cells, raising=False)
    monkeypatch.setattr(ecb, "count_alignments", _fake_count)
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    with caplog.at_level("ERROR", logger="alntools.utils"):
        with pytest.raises(KeyError, match="CELL_NOPE"):
            bin_utils.ecquant_cells(MS, out, samples=["CELL_NOPE"], report=rep)
    assert "Error: sample CELL_NOPE is not in" in caplog.text and not os.path.exists(out) and not os.path.exists(rep)
    m = bin_utils.ecload(MS)
    aln = qchk.Problem.of(m).aln()
    h, t = (int(x) for x in np.argwhere(aln > 0)[0])
    m.lengths[t, h] = 0                                         # alignments and no length
    bad = str(tmp_path / "bad.bin")
    bin_utils.ecsave2(bad, m)
    caplog.clear()
    with caplog.at_level("ERROR", logger="alntools.utils"):
        with pytest.raises(ValueError, match="target %s haplotype %s has alignments and length 0" % (m.lname[t], m.hname[h])):
            bin_utils.ecquant_cells(bad, out, samples=[m.sname[0]], use_lengths=True, report=rep)
    assert "Error: target" in caplog.text and not os.path.exists(out) and not os.path.exists(rep)
    bin_utils.ecquant_cells(bad, out, samples=[m.sname[0]], max_iters=2)                    # without -l the lengths are not looked at


def test_the_one_gpu_command_imports_no_pytorch():
    import sys
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    code = ("import sys; from alntools_amd import cli, bin_utils, ecb; assert hasattr(cli, 'ecquant_cells') and hasattr(bin_utils, 'ecquant_cells') "
            "and hasattr(ecb, 'quantify_cells') and hasattr(ecb, 'cell_support'); print('torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr
