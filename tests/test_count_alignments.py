"""count-alignments and ecdump without a GPU: the numpy checker against the reference's recorded arrays, the table writer, ecdump's log
lines, the command line's listing and the C ABI's declarations.  (The counting itself: ``test_gpu_count_alignments.py``.)"""
import json
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, utils

import counts_checker

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "counts_cases.json")))
COUNTED = [c for c in CASES["cases"] if c["aln"] is not None]


def test_fixture_holds_the_cases_the_feature_is_checked_on():
    assert [c["bin"] for c in COUNTED] == ["g1_edge.bin", "g1_edge_targets.bin", "g2_c1.bin", "g5_binwalk.bin", "gt_h8_in.bin", "gt_c1.out.bin"]
    ms = [c for c in CASES["cases"] if c["aln"] is None]
    assert [c["bin"] for c in ms] == ["g4_multi_min0.bin"] and ms[0]["raises"] == "IndexError"      # the reference cannot count it


@pytest.mark.parametrize("case", COUNTED, ids=[c["bin"] for c in COUNTED])
def test_checker_equals_the_reference(case):
    m = bin_utils.ecload(os.path.join(GOLDEN, case["bin"]))
    assert [m.num_haplotypes, m.num_loci] == case["shape"]
    got = counts_checker.count(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    for name, g, e in zip(("aln", "uniq", "locus_uniq"), got, counts_checker.golden_arrays(case)):
        assert g.dtype == np.int64 and np.array_equal(g, e), name
    assert got[0].any()


def test_checker_multisample_weights():
    """All samples: the row sums of N; one sample: its column; an EC listed twice in a column has its counts added; absent ECs weigh 0."""
    pn, xn, dn = [0, 2, 2, 5], [0, 3, 1, 3, 3], [5, 7, 2, 10, 100]
    assert counts_checker.weights(5, pn, xn, dn).tolist() == [5, 2, 0, 117, 0]
    assert counts_checker.weights(5, pn, xn, dn, sample=0).tolist() == [5, 0, 0, 7, 0]
    assert counts_checker.weights(5, pn, xn, dn, sample=1).tolist() == [0, 0, 0, 0, 0]
    assert counts_checker.weights(5, pn, xn, dn, sample=2).tolist() == [0, 2, 0, 110, 0]
    # rows: {t0: A}, {t0: AB}, {t1: B, t2: A}, {t2: B}, {}
    aln, uniq, lu = counts_checker.count([0, 1, 2, 4, 5, 5], [0, 0, 1, 2, 2], [1, 3, 2, 1, 2], 3, 2, pn, xn, dn)
    assert aln.tolist() == [[5 + 2, 0, 0], [2, 0, 117]] and uniq.tolist() == [[5, 0, 0], [0, 0, 117]] and lu.tolist() == [7, 0, 117]


def test_table_writer_g1_edge():
    case = COUNTED[0]
    m = bin_utils.ecload(os.path.join(GOLDEN, case["bin"]))
    aln, uniq, lu = counts_checker.golden_arrays(case)
    lines = bin_utils.counts_table(m.lname, m.hname, aln, uniq, lu).split("\n")
    assert lines[-1] == "" and len(lines) == m.num_loci + 2
    assert lines[0].split("\t") == ["locus"] + ["aln_" + h for h in m.hname] + ["uniq_" + h for h in m.hname] + ["locus_uniq"]
    for t in range(m.num_loci):
        f = lines[1 + t].split("\t")
        assert f[0] == m.lname[t]
        assert f[1:] == [repr(float(v)) for v in list(aln[:, t]) + list(uniq[:, t]) + [lu[t]]]
        assert all(x.endswith(".0") for x in f[1:])                   # the text of the reference's float64 sums: 12.0
    assert any(float(x) > 0 for l in lines[1:-1] for x in l.split("\t")[1:])


class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append([record.levelname, record.getMessage()])


@pytest.mark.parametrize("case", CASES["cases"], ids=[c["bin"] for c in CASES["cases"]])
def test_ecdump_lines_equal_the_reference(case):
    cap = _Capture()
    log = utils.get_logger()
    level = log.level
    log.addHandler(cap)
    log.setLevel(logging.DEBUG)
    try:
        bin_utils.ecdump(os.path.join(GOLDEN, case["bin"]))
    finally:
        log.removeHandler(cap)
        log.setLevel(level)
    got = [[lvl, msg.replace(GOLDEN, CASES["golden"])] for lvl, msg in cap.lines if lvl in ("INFO", "ERROR")]
    assert got == case["ecdump"] and len(got) == 7


def test_ecdump_needs_no_ecb():
    """``bin_utils.ecdump`` in a fresh interpreter: neither the libecb binding nor PyTorch is imported."""
    code = "from alntools_amd import bin_utils, utils; utils.configure_logging(1); bin_utils.ecdump(%r)" % os.path.join(GOLDEN, "g1_edge.bin")
    r = subprocess.run([sys.executable, "-X", "importtime", "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
    assert "alntools_amd.bin_utils" in imported and "alntools_amd.ecb" not in imported and "torch" not in imported
    assert "Number of ECs (or reads):" in r.stderr


def test_cli_help_lists_both_commands():
    from click.testing import CliRunner
    from alntools_amd import cli
    out = CliRunner().invoke(cli.cli, ["--help"]).output
    assert re.search(r"^\s+count-alignments\s", out, re.M) and re.search(r"^\s+ecdump\s", out, re.M)
    out = CliRunner().invoke(cli.cli, ["count-alignments", "--help"]).output
    assert "ec_file" in out and "out_file" in out and "--sample" in out and "--verbose" in out


def test_header_declares_and_library_exports_both_entry_points():
    """``include/ecb.h`` declares them through ``ecb_count.h``, which it includes; ``libecb.so`` exports them; the ABI is still 4."""
    hdr = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert re.findall(r"#define ECB_ABI_VERSION\s+(\d+)", hdr) == ["4"]
    assert re.findall(r'^#include "(ecb_\w+\.h)"', hdr, re.M) == ["ecb_count.h"]
    sub = open(os.path.join(ROOT, "include", "ecb_count.h")).read()
    assert set(re.findall(r"^int (ecb_[a-z_]+)\(", sub, re.M)) == set(ecb.COUNT_SYMBOLS)
    lib = ecb.load()
    for s in ("ecb_count_alignments_device", "ecb_count_alignments"):
        assert re.search(r"\bint %s\(int device, uint32_t n_ecs, uint32_t n_loci, uint32_t n_haps, uint64_t nnz_a," % s, sub), s
        assert s in ecb.COUNT_SYMBOLS and hasattr(lib, s), s
    # a C compiler sees them through ecb.h alone
    src = "#include \"ecb.h\"\nint (*a)(int, uint32_t, uint32_t, uint32_t, uint64_t, const int32_t*, const int32_t*, const int32_t*, uint32_t, uint64_t, " \
          "const int32_t*, const int32_t*, const int32_t*, int64_t, int64_t*, int64_t*, int64_t*) = ecb_count_alignments;\n" \
          "int (*b)(int, uint32_t, uint32_t, uint32_t, uint64_t, const void*, const void*, const void*, uint32_t, uint64_t, " \
          "const void*, const void*, const void*, int64_t, void*, void*, void*) = ecb_count_alignments_device;\n"
    r = subprocess.run(["cc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refusals_decided_before_a_device_is_touched():
    """Both entry points, as ``(code, ecb_last_error(NULL))``: null pointers, 0 and 32 haplotypes, 0 loci, 0 samples, sizes at the int32
    limits and at the sort's 2^30, a sample outside [-1, n_samples), no such device.  None of them needs a GPU."""
    import ctypes as C
    lib = ecb.load()
    lib.ecb_last_error.restype = C.c_char_p
    buf = (C.c_int64 * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(device=0, n_ecs=2, n_loci=3, n_haps=2, nnz=4, ipa=p, ixa=p, daa=p, n_samples=1, nnz_n=2, ipn=p, ixn=p, dan=p, sample=-1)
    ARG, LIMIT, CONTRACT, NO_DEVICE = -1, -8, -5, -3
    want = [
        (dict(ipa=None), ARG, "bad argument"), (dict(ipn=None), ARG, "bad argument"), (dict(ixa=None), ARG, "bad argument"),
        (dict(dan=None), ARG, "bad argument"), (dict(n_haps=0), ARG, "bad argument"), (dict(n_haps=32), ARG, "bad argument"),
        (dict(n_loci=0), ARG, "bad argument"), (dict(n_samples=0), ARG, "bad argument"),
        (dict(n_ecs=2 ** 31 - 1), LIMIT, "the matrices exceed the .bin format's int32 limits"),
        (dict(nnz_n=2 ** 31), LIMIT, "the matrices exceed the .bin format's int32 limits"),
        (dict(nnz=2 ** 30), LIMIT, "count-alignments: 2^30 non-zeros or more"),
        (dict(sample=1), CONTRACT, "count-alignments: no such sample (1 of 1)"),
        (dict(sample=-2), CONTRACT, "count-alignments: no such sample (-2 of 1)"),
        (dict(device=-1), NO_DEVICE, "no such device"), (dict(device=64), NO_DEVICE, "no such device"),
    ]
    for f in (lib.ecb_count_alignments_device, lib.ecb_count_alignments):
        for change, code, text in want:
            k = dict(ok, **change)
            rc = f(k["device"], k["n_ecs"], k["n_loci"], k["n_haps"], k["nnz"], k["ipa"], k["ixa"], k["daa"], k["n_samples"], k["nnz_n"], k["ipn"],
                   k["ixn"], k["dan"], k["sample"], p, p, p)
            assert (rc, lib.ecb_last_error(None).decode()) == (code, text), (f.__name__, change)
        assert not any(buf)
