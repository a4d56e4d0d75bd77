"""apply-genotypes without a GPU: the genotype / group parser against the masks the reference built, the whole command with the
masking done by the numpy checker against the reference's bytes, and every error case (tests/golden/make_golden_gt.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, utils

import gt_checker

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cases(golden_dir, ok):
    d = json.load(open(os.path.join(golden_dir, "gt_cases.json")))
    return [c for c in d["cases"] if (c["out"] is not None) == ok]


def _path(golden_dir, tmp_path, p):
    return p.replace("<tmp>", str(tmp_path)) if p.startswith("<tmp>") else os.path.join(golden_dir, p)


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture
def checker_masking(monkeypatch):
    calls = []

    def apply_mask(indptr, indices, data, mask, n_haps, device=0):
        calls.append(n_haps)
        return gt_checker.mask_csr(indptr, indices, data, mask)

    monkeypatch.setattr(ecb, "apply_mask", apply_mask)
    return calls


class _Lines(object):
    def __init__(self):
        import logging

        class H(logging.Handler):
            def emit(s, r):
                self.lines.append((r.levelname, r.getMessage()))
        self.lines, self.h = [], H()

    def __enter__(self):
        log = utils.get_logger()
        self.level = log.level
        log.addHandler(self.h)
        log.setLevel(10)
        return self

    def __exit__(self, *a):
        utils.get_logger().removeHandler(self.h)
        utils.get_logger().setLevel(self.level)


@pytest.mark.parametrize("name", ["c1", "c1_homA", "ms", "h8"])
def test_parser_builds_the_reference_mask(golden_dir, name):
    c = {c["name"]: c for c in _cases(golden_dir, True)}[name]
    m = bin_utils.ecload(os.path.join(golden_dir, c["ec"]))
    gname, groups = bin_utils.load_groups(m, os.path.join(golden_dir, c["grp"]))
    mask = bin_utils.genotype_mask(m, os.path.join(golden_dir, c["gt"]), gname, groups)
    assert mask.dtype == np.uint32 and len(mask) == m.num_loci
    assert mask.tolist() == c["mask"]


@pytest.mark.parametrize("name", ["c1", "c1_homA", "ms", "h8"])
def test_command_with_the_checker_writes_the_reference_bytes(golden_dir, tmp_path, checker_masking, name):
    c = {c["name"]: c for c in _cases(golden_dir, True)}[name]
    out = str(tmp_path / "out.bin")
    with _Lines() as L:
        bin_utils.apply_genotypes(os.path.join(golden_dir, c["ec"]), os.path.join(golden_dir, c["gt"]), os.path.join(golden_dir, c["grp"]), out)
    assert checker_masking, "the masking was not asked for"
    assert _bytes(out) == _bytes(os.path.join(golden_dir, c["out"]))
    info = [m.replace(golden_dir, "<golden>").replace(out, "<golden>/" + c["out"]) for lvl, m in L.lines if lvl == "INFO" and "total time" not in m]
    assert info == c["info"]
    assert not [m for lvl, m in L.lines if lvl == "ERROR"]


def test_the_checker_keeps_empty_rows_and_the_multisample_n(golden_dir):
    c = {c["name"]: c for c in _cases(golden_dir, True)}["c1_homA"]
    a, b = bin_utils.ecload(os.path.join(golden_dir, c["ec"])), bin_utils.ecload(os.path.join(golden_dir, c["out"]))
    assert b.num_reads == a.num_reads and (np.diff(b.indptrA) == 0).sum() > 0
    ms = {c["name"]: c for c in _cases(golden_dir, True)}["ms"]
    a, b = bin_utils.ecload(os.path.join(golden_dir, ms["ec"])), bin_utils.ecload(os.path.join(golden_dir, ms["out"]))
    for k in ("indptrN", "indicesN", "dataN"):
        assert np.array_equal(getattr(a, k), getattr(b, k))


@pytest.mark.parametrize("case", [c["name"] for c in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "gt_cases.json")))["cases"]
                                  if c["out"] is None])
def test_error_case_logs_the_reference_message_and_writes_nothing(golden_dir, tmp_path, checker_masking, case):
    c = {c["name"]: c for c in _cases(golden_dir, False)}[case]
    out = str(tmp_path / "out.bin")
    with _Lines() as L:
        bin_utils.apply_genotypes(_path(golden_dir, tmp_path, c["ec"]), _path(golden_dir, tmp_path, c["gt"]), _path(golden_dir, tmp_path, c["grp"]), out)
    assert [m.replace(str(tmp_path), "<tmp>") for lvl, m in L.lines if lvl == "ERROR"] == c["errors"]
    assert not os.path.exists(out)
    assert not checker_masking


@pytest.mark.parametrize("case", ["err_gene", "err_nogt"])
def test_command_line_error_exits_zero_and_writes_nothing(golden_dir, tmp_path, case):
    c = {c["name"]: c for c in _cases(golden_dir, False)}[case]
    out = str(tmp_path / "out.bin")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    args = [_path(golden_dir, tmp_path, c[k]) for k in ("ec", "gt", "grp")] + [out]
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "apply-genotypes"] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert c["errors"][0].replace("<tmp>", str(tmp_path)) in r.stderr
    assert not os.path.exists(out)


def test_the_abi_declares_the_apply_mask_entries():
    hdr = open(os.path.join(ROOT, "include", "ecb.h")).read()
    for s in ("ecb_apply_mask_device", "ecb_apply_mask"):
        assert s + "(" in hdr and s in ecb.SYMBOLS
    assert ecb.ABI_VERSION == 4
