"""ecquant's hierarchical models per cell without a GPU: the cell model checker (tests/cell_model_checker.py) pinned to the step pairs recorded
from the reference's own factors for five cells of ``g4b_multi_min0.bin`` (``quant_cell_models_cases.json``), the hand-built rows of the
deviation as one-cell problems, the ABI's header, the constants the GPU tests place their shapes on, the command's wiring and its host
refusals.

The tolerance of one step of one cell is ``test_ecquant_models.py``'s, evaluated with the cell's own values.  Nothing cancels, so a result
carries one rounding of 2^-53 per addition in the longest chain of each sum it depends on, plus one per multiplication and division; with
B = the most set bits in one of the cell's rows, L = its longest per-haplotype column, M = the most members of one gene within the cell's
support (Phi_gh has at most M terms, Phi_g M H: no sum is longer than the support allows), R = the most genes in one of its rows:

  model 3   B + L + R + 2 M H + 3          model 1   B + L + R + 2 M H + 2 M + H + 4          model 2   L + R + 2 M H + M + 3 H + 4

roundings on either side; two results agree when they differ by at most that many plus 2, times 2^-52, of the reference's value, entry by
entry, and exactly the same entries are 0 (``CellGrouping.tolerance``).  The checker against the recorded pairs: worst relative difference
5.8e-16, the smallest bound (cell 157: one entry, one gene) 2.7e-15."""
import os
import re
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import cell_model_checker as cm
import cell_quant_checker as cq
import counts_checker
import quant_checker as qchk
import quant_model_checker as mchk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = cm.GOLDEN
SRC = os.path.join(ROOT, "alntools_amd", "csrc", "quant_cells_model.inc")
MS = os.path.join(GOLDEN, "g4b_multi_min0.bin")
GRP = os.path.join(GOLDEN, "quant_model_ms.grp.txt")
#: what the GPU tests import: the thresholds they straddle and the planner's bytes per expanded non-zero
QC_LONG_ROW, QC_LONG_COL, Q_LONG_GENE, TPB = 256, 32, 32, 256
QC_X_BYTES, QC_SLOT_TABLES, QCM_X_BYTES, QCM_COEF_BYTES, QCM_SLOT_BYTES, QCM_SLOT_TABLES = 64, 4, 64, 8, 40, 1


def per_x_bytes(H, model):
    """The device bytes a batch is planned with per expanded non-zero."""
    flat = QC_X_BYTES + QC_SLOT_TABLES * 8 * H
    return flat if model == 4 else flat + QCM_X_BYTES + QCM_SLOT_BYTES + (QCM_COEF_BYTES + QCM_SLOT_TABLES * 8) * H


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


# ---- the checker against the reference ----------------------------------------------------------------------------------------------------
def test_the_recorded_cells_are_the_ones_the_issue_names():
    m, cs, gene, G, qs, z = cm.ms()
    assert [c["cell"] for c in cm.CASES] == [0, 3, 157, 190, 219] and all(c["steps"] == [0, 1, 5] and c["models"] == [1, 2, 3] for c in cm.CASES)
    assert all((c["ec"], c["grp"], c["shape"][:2]) == ("g4b_multi_min0.bin", "quant_model_ms.grp.txt", [30, 2]) for c in cm.CASES)
    flat = {0} | {c["cell"] for c in __import__("json").load(open(os.path.join(GOLDEN, "quant_cells_cases.json")))["cases"]}
    assert flat == {c["cell"] for c in cm.CASES}                       # the five that quant_ms_s0 and quant_cells_cases.json cover
    assert os.path.getsize(os.path.join(GOLDEN, "quant_cell_models.npz")) <= 970265
    assert np.array_equal(gene, bin_utils.gene_ids(m, GRP)[0]) and G == cm.CASES[0]["G"] == 18
    for case in cm.CASES:
        q, pre = qs[case["cell"]], case["prefix"]
        assert len(q.cell.rows) == case["entries"] and (q.p.B, q.p.L, q.M, q.R) == (case["B"], case["L"], case["M"], case["R"])
        assert np.array_equal(counts_checker.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN, case["cell"]), z[pre + "w"])
        for model in cm.MODELS:
            assert np.array_equal(q.p.aln(), z["%sm%d_theta_0" % (pre, model)])          # theta_0 is the cell's aln, exactly
        assert all(np.isfinite(z[k]).all() for k in z if k.startswith(pre))


@pytest.mark.parametrize("case,model,k", cm.TRIPLES, ids=cm.TRIPLE_IDS)
def test_the_cell_checkers_step_reproduces_every_recorded_pair(case, model, k):
    q = cm.ms()[4][case["cell"]]
    theta, ref = cm.pair(cm.ms()[5], case, model, k)
    got, explained = q.step(model, theta)
    bound = q.tolerance(model)
    worst = qchk.agree(got, ref, bound)
    print("cell %d model %d k=%d: worst relative difference %.3g, bound %.3g" % (case["cell"], model, k, worst, bound))
    assert explained == q.cell.W and abs(float(got.sum()) - explained) <= bound * explained
    assert not got[:, np.setdiff1d(np.arange(q.p.T), q.cell.support)].any()


def test_the_cells_bound_is_no_wider_than_the_pooled_one_and_phi_runs_over_the_support_only():
    m, cs, gene, G, qs, z = cm.ms()
    pooled = mchk.Grouping(qchk.Problem.of(m), gene, G)
    for q in qs:
        assert all(q.tolerance(model) <= pooled.tolerance(model) for model in (1, 2, 3, 4))
    # a table positive everywhere: the masked step is the cell's, the unmasked one (the gene's other members counted) is another
    theta = np.full((m.num_haplotypes, m.num_loci), 2.5)
    q = qs[190]
    part = [g for g in np.unique(gene[q.cell.support]) if (gene == g).sum() > (gene[q.cell.support] == g).sum()]
    assert part, "no gene partly inside the support of cell 190"
    for model in (1, 2, 3):
        a, _ = q.step(model, theta)
        b, _ = mchk.step(q, model, theta)
        assert a.tobytes() == q.step(model, q.masked(theta))[0].tobytes()
        assert np.abs(a - b).max() > 1e3 * q.tolerance(model) * a.max()


@pytest.mark.parametrize("name,models,csr,cell,gene,G,theta", cm.deviation_cells(), ids=[d[0] for d in cm.deviation_cells()])
def test_the_deviation_cases_as_one_cell_problems(name, models, csr, cell, gene, G, theta):
    q = cm.CellGrouping(cell, gene, G)
    W = 18
    assert q.cell.W == W and len(q.cell.rows) == 3 and q.cell.support.tolist() == [0, 1, 2]
    for model in (1, 2, 3):
        ours, explained = q.step(model, theta)
        theirs, _ = q.step(model, theta, reference_rule=True)
        assert explained == W and abs(float(ours.sum()) - W) <= q.tolerance(model) * W          # no mass is lost
        assert not ours[theta == 0].any()
        if model in models:
            assert float(theirs.sum()) < W - 1.0                                               # the reference's rule loses part of row 0
        else:
            assert theirs.tobytes() == ours.tobytes()


# ---- the ABI and the constants ------------------------------------------------------------------------------------------------------------
def test_the_abi_declares_the_cell_model_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_quant_cells_model.h")).read()
    quant = open(os.path.join(ROOT, "include", "ecb_quant.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert ecb.QUANT_CELLS_MODEL_SYMBOLS == ("ecb_quantify_cells_model_device", "ecb_quantify_cells_model")
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.QUANT_CELLS_MODEL_SYMBOLS)
    assert len(re.findall(r'^#include "ecb_quant_cells_model\.h"', quant, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.QUANT_CELLS_MODEL_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS) | set(ecb.BUNDLE_SYMBOLS) | set(ecb.SELECT_SYMBOLS)
                                                     | set(ecb.QUANT_SYMBOLS) | set(ecb.QUANT_MODEL_SYMBOLS) | set(ecb.QUANT_CELLS_SYMBOLS))
    assert "over the cell's support only" in hdr
    from alntools_amd import build
    assert any(p.endswith("ecb_quant_cells_model.h") for p in build.inputs()) and any(p.endswith("quant_cells_model.inc") for p in build.inputs())
    # a C compiler sees them through ecb.h alone: ecb_quantify_cells's arguments with n_genes, gene and model directly after budget_bytes
    src = ('#include "ecb.h"\n'
           "int (*a)(int, uint32_t, uint32_t, uint32_t, uint64_t, const int32_t*, const int32_t*, const int32_t*, uint32_t, uint64_t, const int32_t*, "
           "const int32_t*, const int32_t*, const uint8_t*, const double*, const double*, uint32_t, double, uint64_t, uint32_t, const int32_t*, uint32_t, "
           "uint64_t, int64_t*, int32_t*, double*, uint32_t*, double*, int64_t*, uint8_t*) = ecb_quantify_cells_model;\n"
           "int (*b)(int, uint32_t, uint32_t, uint32_t, uint64_t, const void*, const void*, const void*, uint32_t, uint64_t, const void*, "
           "const void*, const void*, const void*, const void*, const void*, uint32_t, double, uint64_t, uint32_t, const void*, uint32_t, "
           "uint64_t, void*, void*, void*, void*, void*, void*, void*) = ecb_quantify_cells_model_device;\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _const(text, kind, name):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;,]+);" % (kind, name), text)
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    return int(defs[0].strip())


def test_constants_the_cell_model_tests_straddle():
    csrc = os.path.join(ROOT, "alntools_amd", "csrc")
    cells, model, mine = (open(os.path.join(csrc, f)).read() for f in ("quant_cells.inc", "quant_model.inc", "quant_cells_model.inc"))
    assert (_const(cells, "u32", "QC_LONG_ROW"), _const(cells, "u32", "QC_LONG_COL"), _const(model, "u32", "Q_LONG_GENE")) == (QC_LONG_ROW, QC_LONG_COL, Q_LONG_GENE)
    assert (_const(cells, "u64", "QC_X_BYTES"), _const(cells, "u64", "QC_SLOT_TABLES")) == (QC_X_BYTES, QC_SLOT_TABLES)
    assert [_const(mine, "u64", n) for n in ("QCM_X_BYTES", "QCM_COEF_BYTES", "QCM_SLOT_BYTES", "QCM_SLOT_TABLES")] == [QCM_X_BYTES, QCM_COEF_BYTES, QCM_SLOT_BYTES,
                                                                                                                       QCM_SLOT_TABLES]
    main = open(os.path.join(csrc, "ecb.hip")).read()
    assert int(re.search(r"constexpr int TPB = (\d+);", main).group(1)) == TPB
    assert main.index('#include "quant_cells.inc"') < main.index('#include "quant_cells_model.inc"') and len(re.findall(r'^#include "quant_cells_model\.inc"', main, re.M)) == 1
    # the thresholds are the ones the kernels branch on; no sum is a float atomic; plain launches
    # (a long group is left to its workgroup where a long gene is: in quant_model.inc's qm_gh_sum, the body k_qm_gh and k_qcm_gh share)
    assert len(re.findall(r"b - a > Q_LONG_GENE", model)) == 1 and "b - a > Q_LONG_GENE" in model.split("void qm_gh_sum(")[1].split("\n}\n")[0]
    assert "qm_gh_sum(gptr, gmem" in mine.split("void k_qcm_gh(")[1].split("\n}\n")[0]
    assert "gptr[g + 1] - gptr[g] > Q_LONG_GENE" in mine and "b - a <= QC_LONG_ROW" in mine and "b - a > QC_LONG_COL" in mine
    assert "atomicAdd(reinterpret_cast<double" not in mine and "unsafeAtomicAdd" not in mine and "hipGraph" not in mine and "atomicAdd(&d" not in mine
    assert per_x_bytes(2, 4) == 128 and per_x_bytes(2, 1) == 128 + 104 + 32


# ---- the command --------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_hands_the_model_and_the_groups_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e = tmp_path / "e.bin"
    e.write_bytes(b"")
    g = tmp_path / "g.txt"
    g.write_text("")
    o = str(tmp_path / "o.tsv")
    seen = []
    monkeypatch.setattr(methods, "ecquant_cells", lambda *a: seen.append(a))
    for argv in (["-M", "1", "-g", str(g)], ["--model", "3", "--groups", str(g), "-i", "7", "-s", "c1"], ["-M", "4", "-g", str(g)], ["-M", "2"], []):
        r = CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o] + argv)
        assert r.exit_code == 0, r.output
    assert seen == [(str(e), o, None, None, False, 1000, 1e-6, None, 1, str(g)), (str(e), o, ["c1"], None, False, 7, 1e-6, None, 3, str(g)),
                    (str(e), o, None, None, False, 1000, 1e-6, None, 4, str(g)), (str(e), o, None, None, False, 1000, 1e-6, None, 2, None),
                    (str(e), o, None, None, False, 1000, 1e-6, None)]
    assert CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o, "-M", "5"]).exit_code == 2
    assert CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o, "-M", "0"]).exit_code == 2
    assert CliRunner().invoke(cli.cli, ["ecquant-cells", str(e), o, "-M", "1", "-g", str(tmp_path / "nope.txt")]).exit_code == 2 and len(seen) == 5
    out = CliRunner().invoke(cli.cli, ["ecquant-cells", "--help"]).output
    assert "--model" in out and "--groups" in out
    # methods hands both on by name; positional callers of the old signature are unaffected
    monkeypatch.undo()
    got = []
    monkeypatch.setattr(bin_utils, "ecquant_cells", lambda *a, **kw: got.append((a, kw)))
    methods.ecquant_cells("a", "b", None, None, False, 5, 1e-3, "r")
    methods.ecquant_cells("a", "b", None, None, False, 5, 1e-3, "r", 2, "g")
    assert [(kw["model"], kw["groups"]) for _, kw in got] == [(4, None), (2, "g")]


def _no_partition(tmp_path):
    """A group file over the targets of MS that lists one target in two groups."""
    lname = cm.ms()[0].lname
    f = tmp_path / "two.grp.txt"
    f.write_text("GA\t%s\t%s\nGB\t%s\n" % (lname[0], lname[1], lname[1]))
    return str(f)


def test_a_model_without_a_group_file_is_refused_by_name_and_writes_nothing(tmp_path, caplog):
    from click.testing import CliRunner
    from alntools_amd import cli
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    for model in (1, 2, 3):
        caplog.clear()
        with caplog.at_level("ERROR", logger="alntools.utils"):
            with pytest.raises(ValueError, match=r"model %d needs a group file \(-g/--groups\)" % model):
                bin_utils.ecquant_cells(MS, out, model=model, report=rep)
        assert "Error: model %d needs a group file" % model in caplog.text and not os.path.exists(out) and not os.path.exists(rep)
    with pytest.raises(ValueError, match="model 7 is not one of 1, 2, 3, 4"):
        bin_utils.ecquant_cells(MS, out, model=7, groups=GRP)
    r = CliRunner().invoke(cli.cli, ["ecquant-cells", MS, out, "-M", "2"])
    assert r.exit_code == 1 and not os.path.exists(out)
    # a group file that is no partition: refused by name before the device is asked for anything
    with pytest.raises(ValueError, match="is in two groups"):
        bin_utils.ecquant_cells(MS, out, model=1, groups=_no_partition(tmp_path))
    assert not os.path.exists(out)


def test_ecquant_cells_with_the_checker_as_the_device_writes_the_checkers_tables(tmp_path, monkeypatch, caplog):
    def no_flat(*a, **kw):
        raise AssertionError("the flat step was asked for")
    monkeypatch.setattr(ecb, "quantify_cells_model", cm.quantify_cells_model, raising=False)
    monkeypatch.setattr(ecb, "quantify_cells", no_flat)
    m, cs, gene, G, qs, z = cm.ms()
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    names = [m.sname[3], m.sname[190]]
    keep = np.isin(np.arange(m.num_samples), [3, 190])
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    for model in (1, 2, 3):
        with caplog.at_level("INFO", logger="alntools.utils"):
            bin_utils.ecquant_cells(MS, out, samples=names, max_iters=4, tol=0.0, report=rep, model=model, groups=GRP)
        ptr, loc, theta, info = cm.quantify_cells_model(*a, gene=gene, n_genes=G, model=model, cell_keep=keep, max_iters=4, tol=0.0)
        assert open(out).read() == bin_utils.cells_table(m.sname, m.lname, m.hname, ptr, loc, theta)
        assert open(rep).read() == bin_utils.cells_report(m.sname, info, keep)
        assert "Estimating abundances of 2 cells (model %d, 18 genes)" % model in caplog.text
        os.remove(out)
    # model 4 with a group file: the flat step, the file not even read
    seen = []
    monkeypatch.setattr(ecb, "quantify_cells", lambda *a, **kw: seen.append(kw) or cq.quantify_cells(*a, **kw))
    bin_utils.ecquant_cells(MS, out, samples=names, max_iters=2, model=4, groups=_no_partition(tmp_path))
    assert len(seen) == 1 and os.path.exists(out)


def test_the_one_gpu_command_still_imports_no_pytorch():
    import sys
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    code = ("import sys; from alntools_amd import cli, bin_utils, ecb; assert hasattr(ecb, 'quantify_cells_model'); print('torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr
