"""ecquant without a GPU: the quant checker (tests/quant_checker.py) pinned to the step pairs recorded from the reference's own ``multiply`` /
``normalize_reads`` / ``sum`` calls (``tests/golden/quant_cases.json``), its run against its single steps, the ABI's header, the command's
wiring, the table writer and the host's refusals.

The tolerance of one step is derived, not measured: every term is non-negative, so nothing cancels, and a result carries at most
B + L + 2 roundings of 2^-53 on either side (B = the most set bits in a row: the sum d[e]; L = the longest per-haplotype column: the sum of
r; the product with scale, the division and the product with phi).  Two results agree when they differ by at most (B + L + 4) 2^-52 of the
reference's value, entry by entry, and exactly the same entries are 0."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import quant_checker as qchk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "quant_cases.json")))["cases"]
PAIRS = [(c, k) for c in CASES for k in c["steps"]]
_loaded = {}


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    """The command sets the package logger's level (``-v``); tests after these ones find it as it was."""
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


def load_case(case):
    """(ECMatrices, Problem, the .npz's arrays, scale or None) of one recorded case, loaded once."""
    if case["name"] not in _loaded:
        m = bin_utils.ecload(os.path.join(GOLDEN, case["ec"]))
        z = dict(np.load(os.path.join(GOLDEN, case["npz"])))
        _loaded[case["name"]] = (m, qchk.Problem.of(m, case["sample"]), z, z.get("scale"))
    return _loaded[case["name"]]


def test_the_recorded_cases_are_the_ones_the_issue_names():
    assert [(c["name"], c["ec"], c["sample"], c["use_lengths"], c["steps"]) for c in CASES] == [
        ("c1", "g2_c1.bin", None, False, [0, 1, 5, 20]), ("ms", "g4b_multi_min0.bin", None, False, [0, 1, 5, 20]),
        ("ms_s0", "g4b_multi_min0.bin", 0, False, [0, 1, 5, 20]), ("c1_gt", "gt_c1.out.bin", None, False, [0, 1, 5, 20]),
        ("h8", "gt_h8_in.bin", None, False, [0, 5]), ("c1_len", "g2_c1.bin", None, True, [0, 1, 5, 20])]
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, c["npz"])) <= 970265


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_checker_sees_the_recorded_weights_shape_and_sum_lengths(case):
    m, p, z, scale = load_case(case)
    assert list(m.shape) == case["shape"] and (p.B, p.L) == (case["B"], case["L"])
    assert np.array_equal(p.w, z["w"])
    assert np.array_equal(p.aln(), z["theta_0"])                 # theta_0 is aln, exactly
    if case["name"] == "c1_gt":
        assert int((~p.has_bit).sum()) == 870                    # its empty rows
    if case["name"] == "h8":
        assert int(np.diff(m.indptrA).max()) == 892 and p.B == 3598        # its long row: 892 non-zeros, 3 598 set bits


@pytest.mark.parametrize("case,k", PAIRS, ids=["%s-k%d" % (c["name"], k) for c, k in PAIRS])
def test_the_checkers_step_reproduces_every_recorded_pair(case, k):
    m, p, z, scale = load_case(case)
    got, explained = qchk.step(p, z["theta_%d" % k], scale)
    worst = qchk.agree(got, z["next_%d" % k], p.tolerance())
    print("%s k=%d: worst relative difference %.3g, bound %.3g" % (case["name"], k, worst, p.tolerance()))
    # theta stays in read units whatever scale is: the sum of theta' is `explained`
    assert abs(float(got.sum()) - explained) <= p.tolerance() * explained and 0 < explained <= p.W


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_the_checkers_run_of_k_steps_is_k_single_steps_bit_for_bit(case):
    m, p, z, scale = load_case(case)
    K = 7
    theta = p.aln()
    for _ in range(K):
        theta, explained = qchk.step(p, theta, scale)
    got, info = qchk.run(p, scale=scale, max_iters=K, tol=0.0)
    assert got.tobytes() == theta.tobytes()
    assert info["n_iter"] == K and info["explained"] == explained and not info["converged"] and info["delta"] > 0
    zero, info0 = qchk.run(p, scale=scale, max_iters=0)
    assert zero.tobytes() == p.aln().tobytes() and info0 == {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": False}
    # fed back through theta_in: the same
    again, _ = qchk.run(p, scale=scale, theta_in=qchk.run(p, scale=scale, max_iters=3, tol=0.0)[0], max_iters=K - 3, tol=0.0)
    assert again.tobytes() == theta.tobytes()


def test_the_checkers_run_stops_at_the_first_small_step_and_an_empty_input_is_converged():
    m, p, z, scale = load_case(CASES[1])
    theta, info = qchk.run(p, tol=1e-9)
    assert info["converged"] and 1 < info["n_iter"] < 1000 and info["delta"] <= 1e-9 * p.W
    short, sinfo = qchk.run(p, max_iters=info["n_iter"] - 1, tol=1e-9)
    assert not sinfo["converged"] and sinfo["n_iter"] == info["n_iter"] - 1 and sinfo["delta"] > 1e-9 * p.W
    e = qchk.Problem([0, 0, 0], [], [], 3, 2, [0, 1], [1], [5])
    theta, info = qchk.run(e)
    assert not theta.any() and theta.shape == (2, 3) and info == {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": True}


def test_a_row_without_abundance_explains_nothing_and_a_stored_zero_mask_counts_as_nothing():
    # rows: 0 -> (t0: h0), 1 -> (t1: h0 h1), 2 -> (t2: stored 0), 3 -> (t0: h1, t1: h0)
    p = qchk.Problem([0, 1, 2, 3, 5], [0, 1, 2, 0, 1], [1, 3, 0, 2, 1], 3, 2, [0, 4], [0, 1, 2, 3], [4, 6, 9, 2])
    assert p.W == 12 and (p.B, p.L) == (2, 2) and p.has_bit.tolist() == [True, True, False, True]
    theta = np.array([[1.0, 0.0, 5.0], [1.0, 0.0, 5.0]])         # target 1 has no abundance: row 1 has d = 0
    got, explained = qchk.step(p, theta)
    assert explained == 6 and got.tolist() == [[4.0, 0.0, 0.0], [2.0, 0.0, 0.0]]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_declares_the_quant_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_quant.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert ecb.QUANT_SYMBOLS == ("ecb_quantify_device", "ecb_quantify")
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.QUANT_SYMBOLS)
    assert len(re.findall(r'^#\s*include "ecb_quant\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.QUANT_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS) | set(ecb.BUNDLE_SYMBOLS) | set(ecb.SELECT_SYMBOLS))
    assert "ecb_quant" not in main.replace('"ecb_quant.h"', "")
    from alntools_amd import build
    assert any(p.endswith("ecb_quant.h") for p in build.inputs()) and any(p.endswith("quant.inc") for p in build.inputs())
    # a C compiler sees them through ecb.h alone
    src = '#include "ecb.h"\nvoid* a = (void*)ecb_quantify; void* b = (void*)ecb_quantify_device;\n'
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the command, the table and the host's refusals ---------------------------------------------------------------------------------------
def test_the_command_line_hands_its_options_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e = tmp_path / "e.bin"
    e.write_bytes(b"")
    o = str(tmp_path / "o.tsv")
    seen = []
    monkeypatch.setattr(methods, "ecquant", lambda *a: seen.append(a))
    r = CliRunner().invoke(cli.cli, ["ecquant", str(e), o, "-s", "cell", "-l", "-i", "25", "-t", "1e-3", "-v"])
    assert r.exit_code == 0, r.output
    r = CliRunner().invoke(cli.cli, ["ecquant", str(e), o, "--use-lengths"])
    assert r.exit_code == 0, r.output
    r = CliRunner().invoke(cli.cli, ["ecquant", str(e), o])
    assert r.exit_code == 0, r.output
    assert seen == [(str(e), o, "cell", True, 25, 1e-3), (str(e), o, None, True, 1000, 1e-6), (str(e), o, None, False, 1000, 1e-6)]
    assert CliRunner().invoke(cli.cli, ["ecquant", str(e), o, "-i", "-1"]).exit_code == 2 and len(seen) == 3

    def boom(*a):
        raise ValueError("no")
    monkeypatch.setattr(methods, "ecquant", boom)
    assert CliRunner().invoke(cli.cli, ["ecquant", str(e), o]).exit_code == 1


def test_the_table_for_a_2_x_3_theta_and_its_numbers_read_back_exactly():
    theta = np.array([[1.5, 0.0, 1.0 / 3.0], [2.0, 1e-30, 7.0]])
    text = bin_utils.quant_table(["tA", "tB", "tC"], ["P", "M"], theta)
    assert text == ("locus\tP\tM\ttotal\n" "tA\t1.5\t2.0\t3.5\n" "tB\t0.0\t1e-30\t1e-30\n"
                    "tC\t0.3333333333333333\t7.0\t7.333333333333333\n")
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    back = np.array([[float(v) for v in r[1:3]] for r in rows]).T
    assert back.tobytes() == theta.tobytes()


def _fake_quantify(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, scale=None, theta_in=None, max_iters=1000,
                   tol=1e-6, device=0):
    p = qchk.Problem(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample)
    return qchk.run(p, scale, theta_in, max_iters, tol)


def _fake_count(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, device=0):
    import counts_checker
    return counts_checker.count(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample)


def test_ecquant_with_the_checker_as_the_device_writes_the_checkers_table(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "quantify", _fake_quantify)
    monkeypatch.setattr(ecb, "count_alignments", _fake_count)            # (-l asks it where the alignments are)
    src, out = os.path.join(GOLDEN, "g4b_multi_min0.bin"), str(tmp_path / "o.tsv")
    m = bin_utils.ecload(src)
    with caplog.at_level("INFO", logger="alntools.utils"):
        bin_utils.ecquant(src, out, sample=m.sname[0], max_iters=9, tol=0.0)
    theta, info = qchk.run(qchk.Problem.of(m, 0), max_iters=9, tol=0.0)
    assert open(out).read() == bin_utils.quant_table(m.lname, m.hname, theta)
    assert "iterations: 9;" in caplog.text and "not converged" in caplog.text and "explained reads: {:,}".format(info["explained"]) in caplog.text
    os.remove(out)
    # -l: scale = 1 / length
    bin_utils.ecquant(src, out, use_lengths=True, max_iters=4, tol=0.0)
    scale = 1.0 / np.asarray(m.lengths).T
    theta, _ = qchk.run(qchk.Problem.of(m), scale=scale, max_iters=4, tol=0.0)
    assert open(out).read() == bin_utils.quant_table(m.lname, m.hname, theta)


def test_the_host_refuses_an_unknown_sample_and_a_length_of_zero_under_l_by_name(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "quantify", _fake_quantify)
    monkeypatch.setattr(ecb, "count_alignments", _fake_count)
    src, out = os.path.join(GOLDEN, "g4b_multi_min0.bin"), str(tmp_path / "o.tsv")
    with caplog.at_level("ERROR", logger="alntools.utils"):
        with pytest.raises(KeyError, match="CELL_NOPE"):
            bin_utils.ecquant(src, out, sample="CELL_NOPE")
    assert "Error: sample CELL_NOPE is not in" in caplog.text and not os.path.exists(out)
    m = bin_utils.ecload(src)
    cell = m.sname[0]                                           # (one cell: some (target, haplotype) has no alignment)
    aln = qchk.Problem.of(m, 0).aln()
    h, t = (int(x) for x in np.argwhere(aln > 0)[0])
    hz, tz = (int(x) for x in np.argwhere(aln == 0)[0])
    m.lengths[tz, hz] = 0                                       # no alignments there: scale 0, no refusal
    scale = bin_utils.length_scale(m, aln)
    assert scale[hz, tz] == 0 and scale[h, t] == 1.0 / m.lengths[t, h]
    bad = str(tmp_path / "bad.bin")
    bin_utils.ecsave2(bad, m)
    bin_utils.ecquant(bad, out, sample=cell, use_lengths=True, max_iters=2)
    os.remove(out)
    m.lengths[t, h] = 0                                         # alignments and no length
    bin_utils.ecsave2(bad, m)
    caplog.clear()
    with caplog.at_level("ERROR", logger="alntools.utils"):
        with pytest.raises(ValueError, match="target %s haplotype %s has alignments and length 0" % (m.lname[t], m.hname[h])):
            bin_utils.ecquant(bad, out, sample=cell, use_lengths=True)
    assert "Error: target" in caplog.text and not os.path.exists(out)
    bin_utils.ecquant(bad, out, max_iters=2)                    # without -l the lengths are not looked at


def test_the_one_gpu_command_imports_no_pytorch():
    import sys
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    code = "import sys; from alntools_amd import cli, bin_utils, ecb; assert hasattr(cli, 'ecquant') and hasattr(bin_utils, 'ecquant') and hasattr(ecb, 'quantify'); print('torch' in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr
