#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the apply-genotypes fixtures (``gt_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden.py``: imports the unmodified reference package from ``/root/reference`` with the
stand-ins of ``_standins/`` ahead of it, runs its ``bin_utils.apply_genotypes`` on ``.bin`` inputs with hand-made genotype and
group files, and records data only:

  gt_cases.json        every case: input .bin, genotype / group file, the output .bin (or null), the error the reference logged,
                       and the mask it built (its gtmask[h, t] folded to one u32 per locus, captured at its ``multiply`` call)
  gt_<case>.gt.txt     the genotype files;  gt_<case>.grp.txt  the group files
  gt_<case>.out.bin    what the reference wrote
  gt_h8_in.bin         the 8-haplotype (A - H) input, written by the reference's own ``ecsave2`` from seeded random arrays

    python tests/golden/make_golden_gt.py
"""
from __future__ import print_function

import json
import logging
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402
from scipy.sparse import csr_matrix  # noqa: E402

from alntools import bin_utils, utils  # noqa: E402  (the reference)
from alntools.matrix.AlignmentPropertyMatrix import AlignmentPropertyMatrix as RefAPM  # noqa: E402

TMP = "<tmp>"        # the directory of the files that do not exist, in the recorded messages
GOLDEN = "<golden>"  # this directory, in the recorded messages


class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append((record.levelname, record.getMessage()))


def make_h8_input(path):
    """8 haplotypes A - H, 4 000 targets, 3 000 ECs: most rows short, one in 20 with 100 - 900 loci; masks 1 .. 255; one sample."""
    rng = np.random.default_rng(20261015)
    T, E, H = 4000, 3000, 8
    rows = []
    for e in range(E):
        k = int(rng.integers(100, 901)) if rng.random() < 0.05 else int(rng.integers(1, 12))
        loc = np.sort(rng.choice(T, size=k, replace=False))
        rows.append((loc, rng.integers(1, 256, size=k)))
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
    indices = np.concatenate([r[0] for r in rows])
    data = np.concatenate([r[1] for r in rows])
    apm = types.SimpleNamespace()
    apm.hname = np.array(list("ABCDEFGH"))
    apm.lname = np.array(["TX%05d" % t for t in range(T)])
    apm.sname = np.array(["h8_sample"])
    apm.num_haplotypes, apm.num_loci, apm.num_samples = H, T, 1
    apm.lengths = rng.integers(100, 5000, size=(T, H)).astype(float)
    apm.data = [csr_matrix((((data >> h) & 1).astype(float), indices, indptr), shape=(E, T)) for h in range(H)]
    for d in apm.data:
        d.eliminate_zeros()
    apm.count = rng.integers(1, 50, size=E).astype(float)
    bin_utils.ecsave2(path, apm)


def groups_for(lname, seed, gene_size=(1, 5), left_out=0.1):
    """Genes of consecutive transcripts; a share of transcripts in no gene."""
    rng = np.random.default_rng(seed)
    genes, t, g = [], 0, 0
    while t < len(lname):
        k = int(rng.integers(gene_size[0], gene_size[1] + 1))
        if rng.random() >= left_out:
            genes.append(("G%05d" % g, list(lname[t:t + k])))
        g += 1
        t += k
    return genes


def write_grp(path, genes):
    with open(path, "w") as f:
        for name, txs in genes:
            f.write("\t".join([name] + txs) + "\n")


def write_gt(path, lines, comments=("# sample genotypes", "#gene\tgenotype")):
    with open(path, "w") as f:
        for c in comments:
            f.write(c + "\n")
        for g, gt in lines:
            f.write("{}\t{}\n".format(g, gt))


def genotypes_for(genes, haps, seed, absent=0.2):
    """Het and hom genotypes; a share of the genes absent from the file."""
    rng = np.random.default_rng(seed)
    out = []
    for name, _ in genes:
        if rng.random() < absent:
            continue
        a, b = rng.choice(haps, size=2)
        out.append((name, a + b if rng.random() < 0.5 else a + a))
    return out


def run_case(tmp, name, ec_in, gt_path, grp_path, cases, note):
    out_path = os.path.join(HERE, "gt_%s.out.bin" % name)
    if os.path.exists(out_path):
        os.remove(out_path)
    seen = []
    orig = RefAPM.multiply

    def multiply(self, multiplier, axis=0):
        seen.append(np.array(multiplier, copy=True))
        return orig(self, multiplier, axis=axis)

    RefAPM.multiply = multiply
    cap = _Capture()
    log = utils.get_logger()
    log.addHandler(cap)
    log.setLevel(logging.DEBUG)
    try:
        bin_utils.apply_genotypes(ec_in, gt_path, grp_path, out_path)
    finally:
        log.removeHandler(cap)
        RefAPM.multiply = orig
    errors = [m.replace(tmp, TMP) for lvl, m in cap.lines if lvl == "ERROR"]
    mask = None
    if seen:
        gm = seen[0]
        mask = [int(v) for v in sum(((gm[h] != 0).astype(np.int64) << h) for h in range(gm.shape[0]))]
    rel = lambda p: os.path.basename(p) if p.startswith(HERE) else p.replace(tmp, TMP)   # noqa: E731
    cases.append({"name": name, "note": note, "ec": rel(ec_in), "gt": rel(gt_path), "grp": rel(grp_path),
                  "out": os.path.basename(out_path) if os.path.exists(out_path) else None,
                  "errors": errors, "info": [m.replace(HERE, GOLDEN) for lvl, m in cap.lines if lvl == "INFO" and "total time" not in m],
                  "mask": mask})
    print(name, "->", cases[-1]["out"], errors)


def main():
    tmp = tempfile.mkdtemp()
    cases = []
    g = lambda n: os.path.join(HERE, n)   # noqa: E731
    h8 = g("gt_h8_in.bin")
    make_h8_input(h8)

    # g2_c1: 2 haplotypes, one sample
    m = bin_utils.ecload(g("g2_c1.bin"))
    genes = groups_for(list(m.lname), 1)
    genes.append((genes[3][0], genes[7][1]))                      # a duplicated gene name: the later line counts
    write_grp(g("gt_c1.grp.txt"), genes)
    write_gt(g("gt_c1.gt.txt"), genotypes_for(genes, list(m.hname), 2))
    run_case(tmp, "c1", g("g2_c1.bin"), g("gt_c1.gt.txt"), g("gt_c1.grp.txt"), cases, "het/hom, absent genes, ungrouped transcripts, duplicate gene")
    # one haplotype everywhere: many rows lose everything
    write_gt(g("gt_c1_homA.gt.txt"), [(n, "A") for n, _ in genes], comments=())
    run_case(tmp, "c1_homA", g("g2_c1.bin"), g("gt_c1_homA.gt.txt"), g("gt_c1.grp.txt"), cases, "one haplotype, no comments")

    # g4b: multisample
    m = bin_utils.ecload(g("g4b_multi_min0.bin"))
    genes4 = groups_for(list(m.lname), 3, gene_size=(1, 3), left_out=0.15)
    write_grp(g("gt_ms.grp.txt"), genes4)
    write_gt(g("gt_ms.gt.txt"), genotypes_for(genes4, list(m.hname), 4), comments=("# multisample",))
    run_case(tmp, "ms", g("g4b_multi_min0.bin"), g("gt_ms.gt.txt"), g("gt_ms.grp.txt"), cases, "multisample: N unchanged")

    # 8 haplotypes, rows of up to 900 loci
    m = bin_utils.ecload(h8)
    genes8 = groups_for(list(m.lname), 5, gene_size=(1, 8))
    write_grp(g("gt_h8.grp.txt"), genes8)
    write_gt(g("gt_h8.gt.txt"), genotypes_for(genes8, list(m.hname), 6))
    run_case(tmp, "h8", h8, g("gt_h8.gt.txt"), g("gt_h8.grp.txt"), cases, "8 haplotypes, long rows")

    # errors (on g2_c1): the reference logs the exception and writes nothing
    c1 = g("g2_c1.bin")
    first = genes[0][0]
    err = {
        "err_gene": [(first, "AB"), ("NOPE", "A")],
        "err_hap": [(first, "AZ")],
        "err_hap_before_gene": [("NOPE", "Z")],
        "err_late_comment": [(first, "A"), ("#late", "B")],
        "err_multichar": [(first, "A"), (genes[1][0], "A B")],
    }
    for name, lines in err.items():
        write_gt(g("gt_%s.gt.txt" % name), lines)
        run_case(tmp, name, c1, g("gt_%s.gt.txt" % name), g("gt_c1.grp.txt"), cases, "error")
    with open(g("gt_err_onefield.gt.txt"), "w") as f:
        f.write("#c\n{}\tAB\n{}\t\n".format(first, genes[1][0]))      # an empty genotype: one field after rstrip
    run_case(tmp, "err_onefield", c1, g("gt_err_onefield.gt.txt"), g("gt_c1.grp.txt"), cases, "error")
    with open(g("gt_err_blankline.gt.txt"), "w") as f:
        f.write("{}\tAB\n\n".format(first))
    run_case(tmp, "err_blankline", c1, g("gt_err_blankline.gt.txt"), g("gt_c1.grp.txt"), cases, "error")
    with open(g("gt_err_tx.grp.txt"), "w") as f:
        f.write("{}\t{}\tTX_NOPE\n".format(first, genes[0][1][0]))
    run_case(tmp, "err_tx", c1, g("gt_c1.gt.txt"), g("gt_err_tx.grp.txt"), cases, "error")
    with open(g("gt_err_emptygroup.grp.txt"), "w") as f:
        f.write("{}\n".format(first))
    write_gt(g("gt_err_emptygroup.gt.txt"), [(first, "A")])
    run_case(tmp, "err_emptygroup", c1, g("gt_err_emptygroup.gt.txt"), g("gt_err_emptygroup.grp.txt"), cases, "error")
    run_case(tmp, "err_nogt", c1, os.path.join(tmp, "missing.gt.txt"), g("gt_c1.grp.txt"), cases, "error")
    run_case(tmp, "err_nogrp", c1, g("gt_c1.gt.txt"), os.path.join(tmp, "missing.grp.txt"), cases, "error")

    with open(g("gt_cases.json"), "w") as f:
        json.dump({"tmp": TMP, "golden": GOLDEN, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
